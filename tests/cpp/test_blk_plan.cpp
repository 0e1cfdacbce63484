// CPU check of the blocked stage 1's launch sizing (svdsolver_amd/csrc/
// brd_blk_plan.h): the conditions the kernels rely on, over a sweep of sizes,
// targets and switches.  No HIP; compiled and run by tests/test_blk_plan.py.
#include "brd_blk_plan.h"

#include <cstdio>
#include <vector>

using namespace brd::blk;

static long g_checks = 0, g_fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        ++g_checks;                                        \
        if (!(cond)) {                                     \
            if (++g_fails <= 20) {                         \
                printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

static const int kSizes[] = {1, 31, 32, 33, 64, 128, 160, 255, 256, 257, 1024, 8192, 16383};
static const int kTargets[] = {1, 32, 112, 224, 256, 304};

// ---- the read passes ------------------------------------------------------------
static void check_rpass_dma(int K, int M, bool virt, size_t elem, const S1Launch &lc) {
    const RpPlan p = rpass_plan(true, K, M, virt, elem, kKsMax, lc);
#define RP_AT "K=%d M=%d virt=%d elem=%zu target=%d lean=%d", K, M, (int)virt, elem, lc.target, (int)lc.lean
    CHECK(p.wst >= 1, RP_AT);
    CHECK(p.kper == 0, RP_AT);
    CHECK(p.mtiles == (M + kMT - 1) / kMT && p.tiles == p.mtiles + (virt ? 1 : 0), RP_AT);
    CHECK((long)p.ns * rpass_stage_k(elem) >= K && (long)(p.ns - 1) * rpass_stage_k(elem) < K, RP_AT);
    CHECK(p.nvirt == (virt ? p.ksplit : 0), RP_AT);
    if (p.wst < 1) return;
    // the kernel's deal: workgroup w takes stages [w wst, (w + 1) wst) of the
    // tiles' stages laid end to end (tile t: [t ns, (t + 1) ns))
    const long tot = (long)p.tiles * p.ns;
    std::vector<int> cover((size_t)tot, 0), touch((size_t)p.tiles, 0);
    long runs = 0;
    for (long u = 0; u < tot; u += p.wst, ++runs) {
        const long end = std::min(tot, u + p.wst);
        for (long x = u; x < end; ++x) ++cover[(size_t)x];
        for (long t = u / p.ns; t <= (end - 1) / p.ns; ++t) ++touch[(size_t)t];
    }
    bool once = true;
    for (long x = 0; x < tot; ++x) once = once && cover[(size_t)x] == 1;
    CHECK(once, RP_AT);
    CHECK(p.grid == runs, RP_AT);
    int most = tot > 0 ? 0 : 1;
    for (int t = 0; t < p.tiles; ++t) most = std::max(most, touch[(size_t)t]);
    CHECK(most == p.ksplit, RP_AT);
    CHECK(p.ksplit <= kKsMax, RP_AT);
}

static void check_rpass_reg(int K, int M, bool virt, size_t elem, const S1Launch &lc) {
    const RpPlan p = rpass_plan(false, K, M, virt, elem, kKsMax, lc);
    CHECK(p.tiles == 0 && p.ns == 0 && p.wst == 0, RP_AT);
    CHECK(p.kper > 0 && p.kper % 8 == 0, RP_AT);
    CHECK((long)p.ksplit * p.kper >= K && (long)(p.ksplit - 1) * p.kper < K, RP_AT);
    CHECK(p.ksplit >= 1 && p.ksplit <= kKsMax, RP_AT);
    CHECK(p.nvirt == (virt ? p.ksplit : 0), RP_AT);
    CHECK(p.grid == (p.mtiles + (virt ? 1 : 0)) * p.ksplit, RP_AT);
#undef RP_AT
}

static void sweep_rpass() {
    for (int K : kSizes)
        for (int M : kSizes)
            for (int virt = 0; virt < 2; ++virt)
                for (size_t elem : {(size_t)4, (size_t)8})
                    for (int target : kTargets)
                        for (int lean = 0; lean < 2; ++lean) {
                            S1Launch lc;
                            lc.target = target;
                            lc.overlap = lc.lean = lean != 0;
                            check_rpass_dma(K, M, virt != 0, elem, lc);
                            check_rpass_reg(K, M, virt != 0, elem, lc);
                        }
}

// ---- the block update -----------------------------------------------------------
static void check_blkupd(int tiles_r, int tiles_c, int target, bool half, bool xcd) {
    S1Launch lc;
    lc.upd_target = target;
    lc.blkupd_half = half;
    lc.blkupd_xcd = xcd;
    const int ntiles = tiles_r * tiles_c;
    const UpdPlan u = blkupd_plan(ntiles, tiles_c, lc);
#define UP_AT "tiles %d x %d target=%d half=%d xcd=%d", tiles_r, tiles_c, target, (int)half, (int)xcd
    CHECK(u.nh % 2 == 0 && u.nh >= 0 && u.nfull >= 0, UP_AT);
    CHECK(u.nfull + u.nh / 2 == ntiles, UP_AT);
    CHECK(u.grid >= 1 && u.grid <= target, UP_AT);
    CHECK(u.grid <= u.nfull + u.nh, UP_AT);
    if (!half) CHECK(u.nh == 0, UP_AT);
    if (!xcd) CHECK(u.xsr == 0 && u.xsc == 0, UP_AT);
    if (u.xsr > 0) {
        CHECK(u.xsr * u.xsc == u.grid / 8, UP_AT);
        CHECK(u.grid % 32 == 0 && u.nfull >= u.grid && tiles_r >= 4 && tiles_c >= u.grid / 32, UP_AT);
        CHECK(u.xsr == 4 && u.xsc == u.grid / 32, UP_AT);
    } else {
        CHECK(u.xsc == 0, UP_AT);
    }
    // blkupd_tile: one to one onto tiles_r x tiles_c
    GemmArgs g{};
    g.tiles_c = tiles_c;
    g.ntiles = ntiles;
    g.nfull = u.nfull; g.nh = u.nh; g.xsr = u.xsr; g.xsc = u.xsc;
    std::vector<int> seen((size_t)ntiles, 0);
    bool in_range = true;
    for (int q = 0; q < ntiles; ++q) {
        int tr = -1, tc = -1;
        blkupd_tile(g, q, tr, tc);
        if (tr < 0 || tr >= tiles_r || tc < 0 || tc >= tiles_c) { in_range = false; continue; }
        ++seen[(size_t)tr * tiles_c + tc];
    }
    bool once = in_range;
    for (int t = 0; t < ntiles; ++t) once = once && seen[(size_t)t] == 1;
    CHECK(once, UP_AT);
#undef UP_AT
}

static long g_xcd_cases = 0, g_ragged_xcd_cases = 0;
static void sweep_blkupd() {
    for (int tiles_r = 1; tiles_r <= 70; ++tiles_r)
        for (int tiles_c = 1; tiles_c <= 70; ++tiles_c)
            for (int target : {32, 224, 256})
                for (int half = 0; half < 2; ++half)
                    for (int xcd = 0; xcd < 2; ++xcd) {
                        check_blkupd(tiles_r, tiles_c, target, half != 0, xcd != 0);
                        S1Launch lc;
                        lc.upd_target = target; lc.blkupd_half = half != 0; lc.blkupd_xcd = xcd != 0;
                        const UpdPlan u = blkupd_plan(tiles_r * tiles_c, tiles_c, lc);
                        if (u.xsr > 0) {
                            ++g_xcd_cases;
                            if (tiles_c % u.xsc != 0) ++g_ragged_xcd_cases;
                        }
                    }
    // the sweep must have reached the super-tile order, ragged strips included
    CHECK(g_xcd_cases > 0 && g_ragged_xcd_cases > 0, "xcd cases %ld ragged %ld", g_xcd_cases, g_ragged_xcd_cases);
    // blkupd_tile with super-tiles of any shape (not only those blkupd_plan
    // picks): every xsr x xsc that fits the grid of tiles
    for (int tiles_r = 1; tiles_r <= 12; ++tiles_r)
        for (int tiles_c = 1; tiles_c <= 12; ++tiles_c)
            for (int xsr = 1; xsr <= tiles_r; ++xsr)
                for (int xsc = 1; xsc <= tiles_c; ++xsc) {
                    GemmArgs g{};
                    g.tiles_c = tiles_c; g.ntiles = tiles_r * tiles_c; g.xsr = xsr; g.xsc = xsc;
                    std::vector<int> seen((size_t)g.ntiles, 0);
                    bool ok = true;
                    for (int q = 0; q < g.ntiles; ++q) {
                        int tr = -1, tc = -1;
                        blkupd_tile(g, q, tr, tc);
                        if (tr < 0 || tr >= tiles_r || tc < 0 || tc >= tiles_c) { ok = false; continue; }
                        ++seen[(size_t)tr * tiles_c + tc];
                    }
                    for (int t = 0; t < g.ntiles; ++t) ok = ok && seen[(size_t)t] == 1;
                    CHECK(ok, "tiles %d x %d super-tiles %d x %d", tiles_r, tiles_c, xsr, xsc);
                }
}

// ---- the prep kernels -------------------------------------------------------------
static void sweep_prep() {
    const int zfills[] = {0, 1, 256, 300, 20000};
    for (int items : {0, 1, 31, 32, 33, 63, 64, 65, 160, 255, 256, 257, 1024, 8192, 16383})
        for (int zfill : zfills)
            for (int target : kTargets)
                for (int lean = 0; lean < 2; ++lean)
                    for (int mode = -1; mode <= 1; ++mode) {
                        S1Launch lc;
                        lc.target = target;
                        lc.overlap = lc.lean = lean != 0;
                        lc.prep_split = mode;
                        const PrepPlan p = prep_plan(items, zfill, lc);
                        const int per = p.split ? kPI : 2 * kPI;
#define PP_AT "items=%d zfill=%d target=%d lean=%d mode=%d", items, zfill, target, lean, mode
                        CHECK(p.split == 0 || p.split == 1, PP_AT);
                        CHECK(p.grid >= 1 && (long)p.grid * per >= std::max(items, zfill), PP_AT);
                        CHECK((long)(p.grid - 1) * per < std::max(std::max(items, zfill), 1), PP_AT);   // no idle workgroup
                        // "under lean, split is 0" is the rule with BRD_PREP_SPLIT unset (mode < 0);
                        // the sweep adds the two forced modes, which override it by design (A/B):
                        // mode 1 under lean gives split 1 and is checked as such, not excluded
                        if (mode == 0) CHECK(p.split == 0, PP_AT);
                        if (mode == 1) CHECK(p.split == 1, PP_AT);
                        if (mode < 0 && lean) CHECK(p.split == 0, PP_AT);   // the automatic rule under lean
                        if (mode < 0 && p.split) CHECK(p.grid <= target, PP_AT);   // splits only while it fits
#undef PP_AT
                    }
}

int main() {
    sweep_rpass();
    sweep_blkupd();
    sweep_prep();
    printf("%ld checks, %ld failed\n", g_checks, g_fails);
    if (g_fails) return 1;
    printf("ALL OK\n");
    return 0;
}
