// Blocked stage 1: the block's delayed rank-256 update k_blkupd (gfx950).
#include "brd_blk.h"

#include <algorithm>
#include <cstdlib>

namespace brd {
namespace blk {

// ==========================================================================
// k_blkupd: C[r][c] -= sum_{k < 256} Lw[r][k] RwT[k][c] for r >= r0, c >= c0:
// the block's delayed rank-256 update on the matrix cores.  Workgroup tile
// 128 x 128 (4 waves of 64 x 64: 16 accumulator tiles of 16 x 16), K in
// chunks of 16 through double-buffered LDS (Lw: pair-swizzled [kp][r][2];
// RwT: [k][c] with a 144-element pitch), the C tile in the accumulators.
// ==========================================================================
template <typename T>
struct GemmLds {
    T a[2][kGKC * kGM];     // Lw tile, pair-swizzled
    T b[2][kGKC * kGBP];    // RwT tile
};

template <typename T>
__global__ void __launch_bounds__(kGT, 2) k_blkupd(GemmArgs a) {
    typedef typename G2<T>::v2 v2;
    typedef typename Mf<T>::v4 v4;
    __shared__ GemmLds<T> L;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = lane >> 4, l15 = lane & 15;
    const int tr = blockIdx.x / a.tiles_c, tc = blockIdx.x % a.tiles_c;
    const int r0 = tr * kGM, c0 = tc * kGM;
    const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
    T *C = (T *)a.C;
    const T *Lw = (const T *)a.Lw;
    const T *RwT = (const T *)a.RwT;

    // C tile into the accumulators
    v4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = r0 + wr + 16 * i + Mf<T>::crow(q, g), cc = c0 + wc + 16 * j + l15;
                acc[i][j][g] = (r < a.rows && cc < a.cols) ? C[(size_t)r * a.ldc + cc] : (T)0;
            }

    // per chunk: Lw 128 x 16 (1024 granules), RwT 16 x 128 (1024 granules): 4 + 4 per thread
    auto load = [&](int k0, v2 (&ga)[4], v2 (&gb)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + kGT * i;
            const int r = e >> 3, kp = e & 7;
            const int rg = r0 + r;
            ga[i] = rg < a.rows ? *(const v2 *)(Lw + (size_t)rg * 256 + k0 + 2 * kp) : v2{(T)0, (T)0};
            const int k = e >> 6, cp = e & 63;
            const int cg = c0 + 2 * cp;
            v2 v = {(T)0, (T)0};
            if (cg < a.cols) {
                const T *p = RwT + (size_t)(k0 + k) * a.ldr + cg;
                if (cg + 1 < a.cols) v = *(const v2 *)p; else v.x = p[0];
            }
            gb[i] = v;
        }
    };
    auto stage = [&](int buf, const v2 (&ga)[4], const v2 (&gb)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + kGT * i;
            const int r = e >> 3, kp = e & 7;
            // negated: the MFMA adds A B to the C tile
            *(v2 *)&L.a[buf][2 * (kp * kGM + (r ^ kp))] = v2{-ga[i].x, -ga[i].y};
            const int k = e >> 6, cp = e & 63;
            *(v2 *)&L.b[buf][k * kGBP + 2 * cp] = gb[i];
        }
    };
    const int nc = a.K / kGKC;
    v2 ga[4], gb[4];
    load(0, ga, gb);
    for (int c = 0; c < nc; ++c) {
        stage(c & 1, ga, gb);
        lds_barrier();
        if (c + 1 < nc) load((c + 1) * kGKC, ga, gb);
#pragma unroll
        for (int s = 0; s < kGKC / 4; ++s) {
            const int k = 4 * s + q, kp = k >> 1, hf = k & 1;
            T av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = wr + 16 * i + l15;
                av[i] = L.a[c & 1][2 * (kp * kGM + (r ^ kp)) + hf];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = L.b[c & 1][k * kGBP + wc + 16 * j + l15];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Mf<T>::mma(av[i], bv[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = r0 + wr + 16 * i + Mf<T>::crow(q, g), cc = c0 + wc + 16 * j + l15;
                if (r < a.rows && cc < a.cols) C[(size_t)r * a.ldc + cc] = acc[i][j][g];
            }
}

// --------------------------------------------------------------------------
// k_blkupd_p: the same update as a persistent kernel (VERDICT r3 item 4:
// k_blkupd loads its C tile before the K loop and stores it after, and the two
// workgroups of a CU start in phase, so a good part of every tile had no
// MFMA issue).  One 512-thread workgroup per CU walks tiles t = blockIdx.x,
// + gridDim.x, ...; 8 waves of 64 x 32 (two per SIMD).  The operands reach
// LDS by LDS-DMA (buffer_load_dwordx4 ... lds: no staging registers, rows /
// columns past the matrix read 0), one chunk of K = 16 ahead, continuously
// across tiles.  The accumulators start at zero; the tile's C is loaded into
// registers during its own K loop and the previous tile's result stored
// during it, spread over every chunk (fp64: 2 elements each; fp32: 4), all
// issued after the chunk's DMAs, so a wave's wait for its DMAs never waits
// for C traffic (vmcnt is in order).  One register buffer holds the
// outgoing result until its store is issued, then the incoming C.
// --------------------------------------------------------------------------
constexpr int kGT2 = 512;

// one chunk = 16 KB of Lw (128 rows) and 16 KB of RwT (128 columns): K = 16
// fp64 / 32 fp32; a 16-B DMA granule holds EPV = 2 / 4 consecutive k of one Lw
// row, or EPV columns of one RwT row
template <typename T> constexpr int bu_epv() { return 16 / (int)sizeof(T); }
template <typename T> constexpr int bu_kc() { return 128 / (int)sizeof(T); }
template <typename T> constexpr int bu_bp() { return sizeof(T) == 8 ? kGBP : kGM; }   // RwT row pitch
#ifndef BRD_BLKUPD_DEPTH
#define BRD_BLKUPD_DEPTH 1   // chunks the DMAs run ahead (1 or 2; A/B knob: 2 measured 14.0 vs 13.8 ms)
#endif
constexpr int kBD = BRD_BLKUPD_DEPTH;
constexpr int kBR = kBD == 1 ? 2 : 4;   // LDS buffers: chunk c in buffer c mod kBR (nc is a multiple)
struct GemmLdsP {
    double a[kBR][2048];        // Lw chunk [kg][row ^ kg][EPV] (granules of EPV k)
    double b[kBR > 3 ? kBR : 3][kGKC * kGBP];   // RwT chunk [k][c]: fp64 pitch 144; fp32 pitch 128,
                                                 // granules XOR 4 (k & 3); the half tiles use three
};
// s_waitcnt vmcnt(n') for the counts the block update needs, n' <= n (rounding
// down only ever waits for more)
__device__ __forceinline__ void vmw(int n) {
    if (n >= 20)      asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (n >= 8)  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (n >= 4)  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n >= 2)  asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
#ifndef BRD_BLKUPD_CAFTER
// a chunk's C ops after its first k-step's MFMAs (the barrier's MFMA bubble
// first): k_blkupd_p 12.98 / 12.91 -> 12.76 / 12.72 ms at N = 8192 fp64, same
// box, bitwise the same band (profiles/r04_blkupd_half.txt).  0: before (A/B)
#define BRD_BLKUPD_CAFTER 1
#endif
#ifndef BRD_BLKUPD_CSPREAD
// C traffic over every chunk (fp64: 2 loads + 2 stores a chunk) instead of 4 +
// 4 over the first 8: k_blkupd_p 13.29 -> 13.06 ms at N = 8192 fp64, same box,
// bitwise the same band (profiles/r04_blkupd_half.txt).  0: the first 8 (A/B)
#define BRD_BLKUPD_CSPREAD 1
#endif

#ifndef BRD_BLKUPD_CPOL
#define BRD_BLKUPD_CPOL 2   // cache policy of k_blkupd_p's C loads and stores: nt (streamed once;
                            // keeps L2 for the Lw / RwT strips: s1_blkupd 12.80 -> 12.57 ms at N = 8192 fp64)
#endif
constexpr int kCPol = BRD_BLKUPD_CPOL;
template <typename T>
__global__ void __launch_bounds__(kGT2, 1) k_blkupd_p(GemmArgs a) {
    typedef typename Mf<T>::v4 v4;
    constexpr int E = sizeof(T), EPV = bu_epv<T>(), KC = bu_kc<T>(), BP = bu_bp<T>();
    __shared__ GemmLdsP L;
    // readfirstlane: the wave index (and every DMA's LDS base) is wave-uniform, in SGPRs
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, l15 = lane & 15;
    const int wr = (w >> 2) * 64, wc = (w & 3) * 32;
    T *C = (T *)a.C;
    const T *Lw = (const T *)a.Lw;
    const T *RwT = (const T *)a.RwT;
    constexpr int nc = 256 / KC;     // chunks (K = 256): 16 fp64, 8 fp32
    constexpr int kIOC = BRD_BLKUPD_CSPREAD ? nc : 8;   // chunks carrying C traffic
    constexpr int EPC = 32 / kIOC;                      // accumulator elements per such chunk (flat e = 8 i + 4 j + g)
    constexpr unsigned kOut = 0x80000000u;
    const unsigned lds_a = (unsigned)(uintptr_t)&L.a[0][0], lds_b = (unsigned)(uintptr_t)&L.b[0][0];

    // This wave's DMAs of one chunk into buffer buf: Lw instructions m = 2w,
    // 2w+1 (granule column kg = m >> 1, rows (m & 1) 64 + lane, stored at
    // row ^ kg), RwT instructions i = 2w, 2w+1 (fp64: one k row of 128
    // columns; fp32: rows 2i, 2i + 1, 32 granules each).  Per tile two
    // per-lane byte offsets each (kOut past the matrix), the chunk's k0 in
    // soffset.
    struct Dma {
        u32x4_t ra, rb;
        unsigned va[2], vb[2];
    };
    // Position p of the persistent walk (round p / G, workgroup p % G) -> tile.
    // With super-tiles, a full round's G tiles are dealt so that the G / 8
    // workgroups of one XCD (workgroup b runs on XCD b mod 8) take one
    // super-tile: its Lw rows and RwT columns (xsr + xsc strips of 256 KB)
    // stay in that XCD's 4 MB L2.
    const int G0 = gridDim.x;
    auto tile_at = [&](int p) {
        int q = p;
        if (a.xsr > 0) {
            const int r = p / G0, b = p - r * G0;
            if ((r + 1) * G0 <= a.nfull) q = r * G0 + (b & 7) * (G0 >> 3) + (b >> 3);
        }
        int tr, tc;
        blkupd_tile(a, q, tr, tc);
        return tr * a.tiles_c + tc;
    };
    auto dma_of = [&](int p) {
        Dma d;
        const int t = tile_at(p);
        const int r0 = (t / a.tiles_c) * kGM, c0 = (t % a.tiles_c) * kGM;
        d.ra = rsrc_of(Lw + (size_t)r0 * 256);
        d.rb = rsrc_of(RwT + c0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = 2 * w + u, kg = m >> 1, r = ((m & 1) * 64 + lane) ^ kg;
            d.va[u] = r0 + r < a.rows ? (unsigned)((r * 256 + EPV * kg) * E) : kOut;
            if constexpr (E == 8) {
                d.vb[u] = c0 + 2 * lane < a.cols ? (unsigned)(((2 * w + u) * (int)a.ldr + 2 * lane) * 8) : kOut;
            } else {
                const int k = 2 * (2 * w + u) + (lane >> 5), cg = (lane & 31) ^ (4 * (k & 3));
                d.vb[u] = c0 + 4 * cg < a.cols ? (unsigned)((k * (int)a.ldr + 4 * cg) * 4) : kOut;
            }
        }
        return d;
    };
    auto issue = [&](const Dma &d, int c, int buf) {
        const int k0 = c * KC;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = 2 * w + u, kg = m >> 1;
            dma16(d.ra, d.va[u], (unsigned)(k0 * E),
                  lds_a + (unsigned)(buf * sizeof(L.a[0]) + (kg * kGM + (m & 1) * 64) * 16));
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
            dma16(d.rb, d.vb[u], (unsigned)(k0 * (int)a.ldr * E),
                  lds_b + (unsigned)(buf * sizeof(L.b[0]) + (2 * w + u) * (E == 8 ? kGBP * 8 : 1024)));
    };
    // C through raw buffer accesses relative to the tile origin; the
    // descriptor's num_records ends at the matrix's last row (rows past it
    // read 0 / drop), columns past it get an offset past num_records
    struct Cio {
        __amdgpu_buffer_rsrc_t r;
        unsigned vb[2];
    };
    auto cio_of = [&](int rr0, int cc0, int wrow) {
        Cio o;
        const unsigned long long bytes = (unsigned long long)(a.rows - rr0) * a.ldc * E;
        o.r = __builtin_amdgcn_make_buffer_rsrc(C + (size_t)rr0 * a.ldc + cc0, 0,
                                                (int)(bytes < 0x7fffffffull ? bytes : 0x7fffffffull), 0x00020000);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cl = wc + 16 * j + l15;
            o.vb[j] = cc0 + cl < a.cols ? (unsigned)(((wrow + Mf<T>::crow(q, 0)) * (int)a.ldc + cl) * E) : kOut;
        }
        return o;
    };
    // element (i, j, g) of the lane's accumulators: row wr + 16 i + crow(q, g)
    auto c_at = [&](const Cio &o, int i, int j, int g) {
        return o.vb[j] + (unsigned)((16 * i + Mf<T>::crow(q, g) - Mf<T>::crow(q, 0)) * (int)a.ldc * E);
    };

    v4 acc[4][2];
    T cbuf[4][2][4];
    // acc += this chunk's Lw x RwT (buffer buf)
    auto chunk_mma = [&](int buf, int s0 = 0, int s1 = -1) {   // k-steps [s0, s1) (-1: to the end)
        const T *la = (const T *)L.a[buf], *lb = (const T *)L.b[buf];
        const int se = s1 < 0 ? KC / 4 : s1;
#pragma unroll
        for (int s = s0; s < se; ++s) {
            const int k = 4 * s + q, kg = k / EPV, he = k % EPV;
            T av[4], bv[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = la[EPV * (kg * kGM + ((wr + 16 * i + l15) ^ kg)) + he];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cl = wc + 16 * j + l15;
                if constexpr (E == 8) bv[j] = lb[k * BP + cl];
                else bv[j] = lb[k * BP + 4 * ((cl >> 2) ^ (4 * (k & 3))) + (cl & 3)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = Mf<T>::mma(av[i], bv[j], acc[i][j]);
        }
    };
    bool have_prev = false;
    Cio cprev = cio_of(0, 0, wr);
    static_assert(nc % kBR == 0, "chunk c of every tile sits in buffer c mod kBR");
    static_assert(kIOC <= nc, "C traffic spread over the first kIOC chunks");
    // DMAs run kBD chunks ahead (the next tile's first chunks during this
    // tile's last).  Before reading chunk c a wave waits until no more VMEM
    // ops are outstanding than it issued after chunk c's DMAs (in-order
    // vmcnt): the later chunks' DMAs (4 each) and the C traffic of the chunks
    // in between -- C(x) = EPC loads of this tile's C plus, when there is a
    // previous tile (have_prev), EPC stores of its result, for x < kIOC.  (A
    // count one tile-less first tile gets wrong lets a chunk be read before it
    // landed: round 4 found that with tools/s1_repro.py.)
    const int nfull = a.nh > 0 ? a.nfull : a.ntiles;
    Dma dcur = dma_of(blockIdx.x);
    if (blockIdx.x < nfull) {
#pragma unroll
        for (int c = 0; c < kBD; ++c) issue(dcur, c, c);
    }
    int tix = 0;
    for (int t = blockIdx.x; t < nfull; t += gridDim.x, ++tix) {
        const int tt = tile_at(t);
        const int r0 = (tt / a.tiles_c) * kGM, c0 = (tt % a.tiles_c) * kGM;
        const Cio ccur = cio_of(r0, c0, wr);
        const bool more = t + (int)gridDim.x < nfull;
        const Dma dnext = dma_of(more ? t + gridDim.x : t);
        const int Cx = have_prev ? 2 * EPC : EPC;                         // this tile's C ops per chunk < kIOC
        const int Cp = tix >= 2 ? 2 * EPC : (tix == 1 ? EPC : 0);         // the previous tile's
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = v4{(T)0, (T)0, (T)0, (T)0};
#pragma unroll
        for (int c = 0; c < nc; ++c) {
            {
                // ops issued after chunk c's DMAs: C(x) of the chunks x in
                // [c - kBD, c) (this tile's or, for x < 0, the previous tile's
                // chunk nc + x) and the DMAs of chunks c + 1 .. c + kBD - 1
                int n = 0;
#pragma unroll
                for (int x = c - kBD; x < c; ++x) {
                    if (x >= 0) n += x < kIOC ? Cx : 0;
                    else        n += nc + x < kIOC ? Cp : 0;
                }
#pragma unroll
                for (int y = c + 1; y < c + kBD; ++y) n += (y < nc || more) ? 4 : 0;
                vmw(n);
            }
            __syncthreads();
            // chunk c + kBD (this tile's, or the next tile's) into the buffer read kBR - kBD chunks ago
            {
                const int cn = c + kBD;
                if (cn < nc) issue(dcur, cn, cn % kBR);
                else if (more) issue(dnext, cn - nc, (cn - nc) % kBR);
            }
            if (BRD_BLKUPD_CAFTER) chunk_mma(c % kBR, 0, 1);
            if (c < kIOC) {
                if (have_prev) {
#pragma unroll
                    for (int e = c * EPC; e < (c + 1) * EPC; ++e)
                        buf_st<T, kCPol>(cbuf[e >> 3][(e >> 2) & 1][e & 3], cprev.r, c_at(cprev, e >> 3, (e >> 2) & 1, e & 3));
                }
#pragma unroll
                for (int e = c * EPC; e < (c + 1) * EPC; ++e)
                    cbuf[e >> 3][(e >> 2) & 1][e & 3] = buf_ld<T, kCPol>(ccur.r, c_at(ccur, e >> 3, (e >> 2) & 1, e & 3));
            }
            chunk_mma(c % kBR, BRD_BLKUPD_CAFTER ? 1 : 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) cbuf[i][j][g] -= acc[i][j][g];
        have_prev = true;
        cprev = ccur;
        dcur = dnext;
    }
    if (have_prev) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) buf_st<T, kCPol>(cbuf[i][j][g], cprev.r, c_at(cprev, i, j, g));
    }
    if (a.nh == 0) return;
    // The last round in half tiles (launch_k_blkupd: when it holds at most
    // half as many tiles as the grid has workgroups, e.g. every tile of the
    // small trailing matrices): 64 x 128, eight waves of 32 x 32.  Every C
    // element sees the same MFMA sequence as in a whole tile, so the result
    // is bitwise the whole tile's.  A half tile's chunk is half the MFMA work
    // of a whole one, too little to cover a chunk's DMA latency, so the DMAs
    // run two chunks ahead through three buffers.  Items continue the whole
    // tiles' round-robin order.
    const int G = gridDim.x, b = blockIdx.x;
    const int h0 = b + ((max(0, nfull - b) + G - 1) / G) * G - nfull;
    const int wrh = (w >> 2) * 32;
    auto chunk_mma_h = [&](int slot) {
        const T *la = (const T *)((const char *)&L.a[0][0] + slot * 8192), *lb = (const T *)L.b[slot];
#pragma unroll
        for (int s = 0; s < KC / 4; ++s) {
            const int k = 4 * s + q, kg = k / EPV, he = k % EPV;
            T av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = la[EPV * (kg * 64 + ((wrh + 16 * i + l15) ^ kg)) + he];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cl = wc + 16 * j + l15;
                if constexpr (E == 8) bv[j] = lb[k * BP + cl];
                else bv[j] = lb[k * BP + 4 * ((cl >> 2) ^ (4 * (k & 3))) + (cl & 3)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = Mf<T>::mma(av[i], bv[j], acc[i][j]);
        }
    };
    for (int h = h0; h < a.nh; h += G) {
        const int t = nfull + (h >> 1);   // positions past the full rounds keep their order
        const int tt = tile_at(t);
        const int r0 = (tt / a.tiles_c) * kGM + (h & 1) * 64, c0 = (tt % a.tiles_c) * kGM;
        if (r0 >= a.rows) continue;   // the lower half of a tile past the matrix (uniform)
        // Lw: granule column kg = w of rows lane ^ kg, stored at row lane;
        // RwT as for the whole tile
        const u32x4_t ra = rsrc_of(Lw + (size_t)r0 * 256);
        const unsigned vah = r0 + (lane ^ w) < a.rows ? (unsigned)(((lane ^ w) * 256 + EPV * w) * E) : kOut;
        const Dma d = dma_of(t);
        auto issue_h = [&](int c, int slot) {
            const int k0 = c * KC;
            dma16(ra, vah, (unsigned)(k0 * E), lds_a + (unsigned)(slot * 8192 + w * 64 * 16));
#pragma unroll
            for (int u = 0; u < 2; ++u)
                dma16(d.rb, d.vb[u], (unsigned)(k0 * (int)a.ldr * E),
                      lds_b + (unsigned)(slot * sizeof(L.b[0]) + (2 * w + u) * (E == 8 ? kGBP * 8 : 1024)));
        };
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = v4{(T)0, (T)0, (T)0, (T)0};
        __syncthreads();   // every wave is done with the buffers
        issue_h(0, 0);
        issue_h(1, 1);
        for (int c = 0; c < nc; ++c) {
            // chunk c landed: only chunk c + 1's three DMAs may be younger
            if (c + 1 < nc) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (c + 2 < nc) issue_h(c + 2, (c + 2) % 3);
            chunk_mma_h(c % 3);
        }
        const Cio cc = cio_of(r0, c0, wrh);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) cbuf[i][j][g] = buf_ld<T>(cc.r, c_at(cc, i, j, g));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) buf_st<T>(cbuf[i][j][g] - acc[i][j][g], cc.r, c_at(cc, i, j, g));
    }
}

template <typename T>
void launch_k_blkupd(GemmArgs g, const S1Launch &lc, hipStream_t s, double fl, double by) {
    // rows 16-byte aligned for the DMA granules (fp32: ldr, 256 and the bases
    // multiples of 4 elements)
    const bool al = sizeof(T) == 8 || (g.ldr % 4 == 0 && (uintptr_t)g.RwT % 16 == 0 && (uintptr_t)g.Lw % 16 == 0);
    if (lc.blkupd_p && al) {
        const UpdPlan u = blkupd_plan(g.ntiles, g.tiles_c, lc);
        g.nfull = u.nfull; g.nh = u.nh; g.xsr = u.xsr; g.xsc = u.xsc;
        blk_launch("s1_blkupd", fl, by, k_blkupd_p<T>, dim3(u.grid), dim3(kGT2), s, g);
        return;
    }
    blk_launch("s1_blkupd", fl, by, k_blkupd<T>, dim3(g.ntiles), dim3(kGT), s, g);   // BRD_BLKUPD_P=0 (A/B), unaligned fp32
}
template void launch_k_blkupd<double>(GemmArgs, const S1Launch &, hipStream_t, double, double);
template void launch_k_blkupd<float>(GemmArgs, const S1Launch &, hipStream_t, double, double);

}  // namespace blk
}  // namespace brd
