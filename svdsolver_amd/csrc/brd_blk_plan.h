// Blocked stage 1: how one call's launches are sized.  Pure arithmetic -- no
// HIP, no process state -- checked with a plain C++ compiler by
// tests/cpp/test_blk_plan.cpp.  The launchers fill RpArgs / PrepArgs /
// GemmArgs from the results.
#pragma once

#include <algorithm>
#include <cstddef>

#ifdef __HIPCC__
#define BRD_HD __host__ __device__
#else
#define BRD_HD
#endif

namespace brd {
namespace blk {

constexpr int kMT = 256;   // k_rpass: m per workgroup
constexpr int kPI = 32;    // k_prep: items per workgroup when split: two item waves x two halves of
                           // the K1 range (the correction's MFMA chain over all four SIMDs;
                           // the halves meet in LDS, fixed order); unsplit: 2 kPI items,
                           // four item waves (when the split grid would exceed the CUs)
constexpr int kGM = 128;   // k_blkupd: rows and columns per tile
constexpr int kKsMax = 32;   // most partial slots per tile of a read pass (the partials buffer)

// The sizing of one call's launches is fixed when the call starts and passed
// to every launcher (no hidden per-thread state, no environment reads per
// launch); a switch changed between two library calls takes effect on the next.
struct S1Launch {
    int target = 256;        // workgroups a bandwidth launch may fill (the device's CUs, less a stage-2 reservation)
    bool overlap = false;    // beside a stage-2 reservation (brd_set_overlap: a stream of reductions)
    bool lean = false;       // overlap and max(m, n) <= kLeanMaxN: no prep K split, read passes sized for target / 2
    int upd_target = 256;    // k_blkupd_p's grid: target under overlap, else the device's CUs (not BRD_S1_TARGET)
    // A/B switches (tools/README.md), defaults as initialised here
    int prep_split = -1;     // BRD_PREP_SPLIT: 0 never, 1 always, else the automatic rule
    int prep_gram = 3;       // BRD_PREP_GRAM: bit 0 the QR side, bit 1 the LQ side
    bool prep_generic = false;   // BRD_PREP_GENERIC: the run-time-j prep kernels only
    bool vsum_fold = false;  // BRD_VSUM_FOLD: unset follows overlap
    bool rpass_dma = true;   // BRD_RPASS_DMA: 0 = the register-streaming k_rpass
    bool blkupd_p = true;    // BRD_BLKUPD_P: 0 = the two-per-CU k_blkupd
    bool blkupd_half = true; // BRD_BLKUPD_HALF: the last round in half tiles
    bool blkupd_xcd = false; // BRD_BLKUPD_XCD: per-XCD super-tiles
    double rpx = 1.0;        // BRD_BLK_RPX: scales the read passes' target (>= 0.125)
};

// ---- read pass ------------------------------------------------------------------
// A K x M source in mtiles tiles of kMT (and a virtual tile, 256 wide, when
// virt), split over K into at most ksmax partial slots per tile.
struct RpPlan { int mtiles, tiles, ns, wst, kper, ksplit, nvirt, grid; };   // grid: without the finishing workgroup
inline int rpass_stage_k(size_t elem) { return 128 / (int)elem; }   // k per stage of k_rpass_d
// Beside a stage-2 reservation (lean) a pass is sized for half the CUs: the
// other lanes' kernels run on the rest.  BRD_BLK_RPX scales
// the target further (A/B).  dma: k_rpass_d runs the pass, else k_rpass.
inline RpPlan rpass_plan(bool dma, int K, int M, bool virt, size_t elem, int ksmax, const S1Launch &lc) {
    const int target = std::max(1, (int)((lc.lean ? std::max(1, lc.target / 2) : lc.target) * lc.rpx));
    RpPlan p;
    p.mtiles = (M + kMT - 1) / kMT;
    p.tiles = p.ns = p.wst = 0;
    if (dma) {
        // k_rpass_d: the tiles' stages (32 KB of a 256-wide tile each) laid end
        // to end and dealt in equal runs of wst stages, one run per workgroup
        p.tiles = p.mtiles + (virt ? 1 : 0);
        const int krk = rpass_stage_k(elem);
        p.ns = (K + krk - 1) / krk;
        const long tot = (long)p.tiles * p.ns;
        int wst = (int)((tot + target - 1) / std::max(1, target));
        wst = std::max(wst, std::max(1, 64 / krk));   // >= 64 k per workgroup
        wst = std::max(wst, (p.ns + ksmax - 2) / (ksmax - 1));   // <= ksmax slots per tile
        p.wst = wst;
        p.grid = (int)((tot + wst - 1) / wst);
        p.ksplit = 1;
        for (int t = 0; t < p.tiles; ++t)
            p.ksplit = std::max(p.ksplit, (int)(((long)(t + 1) * p.ns - 1) / wst - ((long)t * p.ns) / wst + 1));
        p.kper = 0;
    } else {
        int ks = std::max(1, target / std::max(1, p.mtiles + 1));
        ks = std::min(ks, std::max(1, K / 64));
        ks = std::min(ks, ksmax);
        p.kper = ((K + ks - 1) / ks + 7) / 8 * 8;
        p.ksplit = (K + p.kper - 1) / p.kper;
        p.grid = (virt ? p.ksplit : 0) + p.mtiles * p.ksplit;
    }
    p.nvirt = virt ? p.ksplit : 0;
    return p;
}

// ---- prep -----------------------------------------------------------------------
// Split K halves (kPI items per workgroup) while that grid fits the CUs the
// stream may use (one workgroup per CU: LDS) and nothing runs beside it, else
// 2 kPI items per workgroup, one K range per wave.  The two forms round the K1
// sums differently, so a matrix's band depends on whether it ran in a stream
// -- as the read passes' split already does.
// BRD_PREP_SPLIT=0 / 1 forces either form for A/B.
// Beside a stage-2 reservation at N <= kLeanMaxN (lean) never split: half the
// workgroups, each holding a whole CU (LDS), leave CUs to the other lanes'
// passes; larger matrices keep the one-at-a-time sizing (the measurements:
// DESIGN.md, "Round 6 against VERDICT r5").
constexpr int kLeanMaxN = 12288;
struct PrepPlan { int split, grid; };
inline PrepPlan prep_plan(int items_, int zfill, const S1Launch &lc) {
    const int items = std::max(items_, zfill);
    const int n1 = (items + kPI - 1) / kPI;
    PrepPlan p;
    p.split = lc.prep_split == 0 ? 0 : (lc.prep_split == 1 || (n1 <= lc.target && !lc.lean)) ? 1 : 0;
    p.grid = std::max(1, p.split ? n1 : (items + 2 * kPI - 1) / (2 * kPI));
    return p;
}

// ---- block update ---------------------------------------------------------------
struct GemmArgs {
    void *C; long ldc;
    int rows, cols;                 // extent of the updated region
    const void *Lw; const void *RwT; long ldr;
    int K;                          // 256
    int tiles_c;                    // column tiles
    int ntiles;                     // tiles
    int nfull = 0, nh = 0;          // k_blkupd_p: nh > 0: tiles [0, nfull) whole, then
                                    // nh half tiles (64 rows) of tiles nfull, nfull + 1, ...
    int xsr = 0, xsc = 0;           // k_blkupd_p: > 0: per-XCD super-tiles of xsr x xsc tiles
                                    // (xsr xsc = grid / 8; blkupd_tile), else row-major order
};

// k_blkupd_p's grid and tile order over ntiles = tiles_r x tiles_c tiles.
struct UpdPlan { int nfull, nh, xsr, xsc, grid; };
inline UpdPlan blkupd_plan(int ntiles, int tiles_c, const S1Launch &lc) {
    const int tgt = lc.upd_target;
    UpdPlan p;
    // The last round in half tiles when it leaves at least half the grid idle
    // (r = ntiles mod tgt, 2 r <= tgt; bitwise the same band).
    // BRD_BLKUPD_HALF=0 turns it off (A/B).
    const int r = ntiles % tgt;
    const bool half = lc.blkupd_half && r > 0 && 2 * r <= tgt;
    p.nfull = half ? ntiles - r : ntiles;
    p.nh = half ? 2 * r : 0;
    p.grid = std::min(p.nfull + p.nh, tgt);
    // per-XCD super-tiles (blkupd_tile) when the grid deals whole rounds evenly
    // over the 8 XCDs: 4 x (grid / 32) tiles, e.g. 4 x 8 on 256 CUs, 4 x 7
    // beside a 32-CU stage-2 reservation.  BRD_BLKUPD_XCD=0 / 1 (A/B)
    const bool xcd = lc.blkupd_xcd && p.grid % 32 == 0 && p.nfull >= p.grid && ntiles / tiles_c >= 4 && tiles_c >= p.grid / 32;
    p.xsr = xcd ? 4 : 0;
    p.xsc = xcd ? p.grid / 32 : 0;
    return p;
}

// k_blkupd_p's tile order.  Tile q of the order -> (tile row, tile column).
// With super-tiles (xsr > 0) the full xsr x xsc blocks come first, each one's
// tiles row-major, then the right strip and the bottom strip row-major;
// otherwise row-major.
BRD_HD inline void blkupd_tile(const GemmArgs &a, int q, int &tr, int &tc) {
    if (a.xsr <= 0) { tr = q / a.tiles_c; tc = q % a.tiles_c; return; }
    const int tiles_r = a.ntiles / a.tiles_c, nsc = a.tiles_c / a.xsc;
    const int Rf = (tiles_r / a.xsr) * a.xsr, Cf = nsc * a.xsc, per = a.xsr * a.xsc;
    if (q < Rf * Cf) {
        const int st = q / per, w = q - st * per;
        tr = (st / nsc) * a.xsr + w / a.xsc;
        tc = (st % nsc) * a.xsc + w % a.xsc;
        return;
    }
    int e = q - Rf * Cf;
    const int rw = a.tiles_c - Cf;
    if (e < Rf * rw) { tr = e / rw; tc = Cf + e % rw; return; }
    e -= Rf * rw;
    tr = Rf + e / a.tiles_c;
    tc = e % a.tiles_c;
}

}  // namespace blk
}  // namespace brd
