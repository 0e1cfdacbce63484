// Stage 1, blocked: dense -> band with a delayed two-sided update (gfx950).
//
// Replaces, for panels of width 32, the per-panel structure of the
// reference's cuda_brd_p1 (svd_cuda_2.cu:1117-1220: QR of the column panel,
// qr_apply_cuda :1039 over the whole trailing matrix, LQ of the row panel,
// lq_apply_cuda :1081 over it again).  Inside a block of nb panels the
// trailing matrix is not written; it is kept as
//
//     A_cur = A - Lw RwT          Lw  (m x 256) = [V_0..V_3 | X_0..X_3]
//                                 RwT (256 x n) = [Y_0..Y_3 | U_0..U_3]^T
//
// (left reflectors I - V_j T_j V_j^T, right reflectors I - U_j S_j U_j^T,
// Y_j = A_cur^T V_j T_j, X_j = A_cur U_j S_j) and updated once per block by
// k_blkupd, a rank-2 nb 32 product on the matrix cores.  Per panel:
//
//   k_rpass (Y)  partial sums of A^T V_j over row splits, and G = Lw^T V_j
//   k_prep (LQ)  Y_j = (A^T V_j - Rw G) T_j, the corrected row panel
//   k_cqr        QR of the row panel's transpose: CholeskyQR2 + Householder
//                reconstruction -> U_j, S_j, the band's L block
//   k_rpass (X)  partial sums of A U_j over column splits, and G = Rw^T U_j
//   k_prep (QR)  X_j = (A U_j - Lw G) S_j, the next corrected column panel
//   k_cqr        QR of the column panel -> V_{j+1}, T_{j+1}, the band's R block
//
// The executable specification (same steps, same workspaces) is
// tests/s1_model.py; DESIGN.md "Stage 1, blocked" has the roofline of each
// kernel.  This file is the host driver; the kernels live in brd_blk_*.hip
// (brd_blk.h), the launch sizing in brd_blk_plan.h.
//
// Every per-call switch is read in one place, s1_launch below, once per
// blk_ge2band / blk_ge2band_dist call (so a switch changed between two calls
// takes effect on the next), into the call's S1Launch:
//   BRD_PREP_SPLIT, BRD_PREP_GRAM, BRD_PREP_GENERIC   the prep kernels
//   BRD_VSUM_FOLD, BRD_RPASS_DMA, BRD_BLK_RPX         the read passes
//   BRD_BLKUPD_P, BRD_BLKUPD_HALF, BRD_BLKUPD_XCD     the block update
// with the overlap flag (api_overlap_active) and the block update's target.
#include "brd.h"
#include "brd_blk.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace brd {
using namespace blk;

// the counters (ints) of the workspace
enum : int {
    kCtrRpass = 16,               // the read pass's arrival counter (RpArgs::counter)
    kCtrDistQr = 40,              // the sharded panel QR's three (CqrArgs::rctr)
    kCtrGram = 64,                // [kCtrGram, + kCW): the prep Gram groups (PrepArgs::gcnt)
    kCtrTotal = kCtrGram + kCW    // all of them: zeroed when a call starts
};
constexpr int kLwCols = 2 * NBMAX * 32;   // columns of Lw, rows of RwT
constexpr int kQt = 32 * 32;              // a 32 x 32 factor (T_j, S_j, Q_t)

// Workspace of the blocked path (elements of T unless noted), carved from one
// device buffer: Lw m x 256, RwT 256 x ldr, partials, Qp, virtual partials
// and result, T/S factors, cluster scratch (doubles) and counters (ints).
struct BlkLayout {
    size_t lw, rwt, ub, part, vpart, vout, qp, tf, cws, ctr, sg, gpp, total;
    long ldr, mp;
};

static BlkLayout blk_layout(int m, int n, size_t elem) {
    BlkLayout L;
    L.ldr = (n + 1) & ~1L;
    L.mp = (std::max(m, n) + 1) & ~1L;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    L.lw = take((size_t)m * kLwCols * elem);
    L.rwt = take((size_t)kLwCols * L.ldr * elem);
    L.ub = take((size_t)n * 32 * elem);
    L.part = take((size_t)kKsMax * 32 * L.mp * elem);
    L.vpart = take((size_t)kKsMax * 32 * kLwCols * elem);
    L.vout = take((size_t)32 * kLwCols * elem);
    L.qp = take((size_t)32 * L.mp * elem);
    L.tf = take((size_t)2 * NBMAX * kQt * elem);
    L.cws = take(cqr_ws_doubles() * sizeof(double));
    L.ctr = take(kCtrTotal * sizeof(int));
    L.sg = take((size_t)(2 * NBMAX + 1) * 32 * sizeof(double));   // s_j per panel and side; zeros
    // the prep kernels' Gram partials (PrepArgs::gram): per workgroup of kPI items
    L.gpp = take((size_t)((std::max(m, n) + kPI - 1) / kPI) * kGramRec * sizeof(double));
    L.total = off;
    return L;
}

size_t blk_ws_bytes(int m, int n, size_t elem) { return blk_layout(m, n, elem).total; }

int blk_columns(int m, int n, int b) {
    // panels of up to kCW x 256 rows (the panel QR's workgroup count)
    if (b != 32 || m > kCW * kCT || n > kCW * kCT) return 0;
    int k0 = 0;
    while (n - k0 >= (NBMAX + 1) * 32) k0 += NBMAX * 32;
    return k0;
}

// the sharded path's tail of the workspace (blk_ge2band_dist below)
struct DistBlk { size_t bc = 0, rec = 0, ar = 0, total = 0; };
static DistBlk dist_blk_layout(int m, int n, int P, int rank, size_t elem) {
    const BlkLayout Ly = blk_layout(m, std::max(dist_local_cols(n, 32, P, rank), 1), elem);
    DistBlk D;
    size_t off = Ly.total;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    D.bc = take((size_t)m * 32 * elem + (kQt + 8) * sizeof(double));       // V' rows, then Q_t + zero flag
    D.rec = take((size_t)3 * P * kCqrRec * sizeof(double));                // the row panel QR's Gram records
    D.ar = take(((size_t)m * 32 + kLwCols * 32 + kQt) * elem);             // G (256 x 32), X rows, then S_j
    D.total = off;
    return D;
}

// Q_t (32 x 32, row-major) and the zero-panel flag of a factored panel, where
// the read pass's finishing workgroup finds them
struct QtSrc { double *qt, *zero; };

// The workspace by name.  r: a row of the matrix, col: a (local) column, j:
// the panel in the block.
template <typename T>
struct BlkWs {
    char *ws;
    BlkLayout L;
    DistBlk D;
    int P;
    BlkWs(void *base, const BlkLayout &L_, const DistBlk &D_ = DistBlk(), int P_ = 1)
        : ws((char *)base), L(L_), D(D_), P(P_) {}

    // Lw [m][256]: row r's V_j at columns [32 j, + 32), X_j at [128 + 32 j, + 32)
    T *Lw(long r = 0) const { return (T *)(ws + L.lw) + (size_t)r * kLwCols; }
    T *V(long r, int j) const { return Lw(r) + 32 * j; }
    T *X(long r, int j) const { return Lw(r) + 32 * (NBMAX + j); }
    // RwT [256][ldr]: rows [32 j, + 32) Y_j^T, rows [128 + 32 j, + 32) U_j^T
    T *RwT(long col = 0) const { return (T *)(ws + L.rwt) + col; }
    T *Y(int j, long col) const { return RwT(col) + (size_t)(32 * j) * L.ldr; }
    T *U(int j, long col) const { return RwT(col) + (size_t)(32 * (NBMAX + j)) * L.ldr; }
    T *Ub(long col) const { return (T *)(ws + L.ub) + (size_t)col * 32; }   // the current U_j, [n][32]
    T *Tf(int j) const { return (T *)(ws + L.tf) + (size_t)kQt * j; }             // T_j
    T *Sf(int j) const { return (T *)(ws + L.tf) + (size_t)kQt * (NBMAX + j); }   // S_j
    void *part() const { return ws + L.part; }     // a read pass's partials
    void *vpart() const { return ws + L.vpart; }   // its virtual tile's partials
    void *vout() const { return ws + L.vout; }     // and their sum G
    void *Qp() const { return ws + L.qp; }         // the corrected panel, transposed [32][mp]
    // the sign vectors of the panels' reconstructions, and 32 zeros ("no correction")
    double *s_q(int j) const { return (double *)(ws + L.sg) + 32 * j; }
    double *s_l(int j) const { return s_q(NBMAX + j); }
    double *s_zero() const { return s_q(2 * NBMAX); }
    // the CholeskyQR scratch (gp1, ew, qt, zero, ...) and the prep kernels' Gram records
    CqrWs cqr() const { return CqrWs((double *)(ws + L.cws)); }
    QtSrc cqr_qt() const { return QtSrc{cqr().qt, cqr().zero}; }
    double *gpp() const { return (double *)(ws + L.gpp); }
    int *ctr(int k = 0) const { return (int *)(ws + L.ctr) + k; }

    // ---- the sharded path ----
    // broadcast buffer: V' (mr rows of 32), then Q_t, then the zero flag
    T *bc_v() const { return (T *)(ws + D.bc); }
    QtSrc bc_qt(int mr) const { double *qt = (double *)(bc_v() + (size_t)mr * 32); return QtSrc{qt, qt + kQt}; }
    size_t bc_bytes(int mr) const { return (size_t)mr * 32 * sizeof(T) + (kQt + 1) * sizeof(double); }
    // record bank b (0: G1 + exponent, 1: G2, 2: G3), rank r's record
    double *rec(int b, int r = 0) const { return (double *)(ws + D.rec) + ((size_t)b * P + r) * kCqrRec; }
    // all-reduce buffer: G (256 x 32), X (mx rows of 32), then the S_j slot
    T *ar_G() const { return (T *)(ws + D.ar); }
    T *ar_X() const { return ar_G() + kLwCols * 32; }
    T *ar_S(int mx) const { return ar_X() + (size_t)mx * 32; }
    size_t ar_gx_count(int mx) const { return (size_t)mx * 32 + kLwCols * 32; }   // G and X
    size_t ar_count(int mx) const { return ar_gx_count(mx) + kQt; }                // all of it
};

size_t blk_dist_ws_bytes(int m, int n, int P, int rank, size_t elem) { return dist_blk_layout(m, n, P, rank, elem).total; }
bool blk_dist_fits(int n, int P) {
    return P >= 1 && P <= kBlkMaxRanks && dist_local_cols(n, 32, P, 0) <= kCW * kCT;   // rank 0 holds the most
}

// The call's launch plan (S1Launch, brd_blk_plan.h): the one place the blocked
// path reads the environment and the library's state.
static S1Launch s1_launch(int m, int n, int target) {
    auto env = [](const char *name, int unset) {
        const char *e = getenv(name);
        return e ? atoi(e) : unset;
    };
    S1Launch lc;
    lc.target = target;
    lc.overlap = api_overlap_active();
    lc.lean = lc.overlap && std::max(m, n) <= kLeanMaxN;
    lc.upd_target = lc.overlap ? api_apply_target() : api_device_cus();
    lc.prep_split = env("BRD_PREP_SPLIT", -1);
    lc.prep_gram = env("BRD_PREP_GRAM", 3);
    lc.prep_generic = env("BRD_PREP_GENERIC", 0) != 0;
    lc.vsum_fold = env("BRD_VSUM_FOLD", lc.overlap) != 0;
    lc.rpass_dma = env("BRD_RPASS_DMA", 1) != 0;
    lc.blkupd_p = env("BRD_BLKUPD_P", 1) != 0;
    lc.blkupd_half = env("BRD_BLKUPD_HALF", 1) != 0;
    lc.blkupd_xcd = env("BRD_BLKUPD_XCD", 0) != 0;
    const char *rpx = getenv("BRD_BLK_RPX");
    lc.rpx = rpx ? std::max(0.125, atof(rpx)) : 1.0;
    return lc;
}

// One read pass: D = B^T S (Y) or S B (X) and the virtual tile's G: what the
// caller gives (the names are RpArgs'; the split comes from rpass_plan)
struct RpCall {
    bool yp;
    const void *src; long ld; int K, M;
    const void *bsrc; long bld;
    const void *vsrc; long vld;
    void *vout = nullptr;                     // G's destination (null: the workspace's)
    int va = 0, vb = 0;
    const FinArgs *fin = nullptr;             // the panel whose reconstruction the pass finishes
    void *pbase = nullptr; long pstride = 0;  // k_vsum's patch: the diagonal of V's / U's top block
    const double *psgn = nullptr;             // gets - s
    bool may_fold = false;                    // the consumers can patch the top block themselves
};

// What every step of one call shares, and the steps both drivers take.
template <typename T>
struct BlkCall {
    T *A; long lda;
    BlkWs<T> W;
    S1Launch lc;
    hipStream_t s;
    int *err;
    int mrows;   // m

    T *a(long r, long col) const { return A + (size_t)r * lda + col; }

    hipError_t reset() const {   // the counters, the zero sign vector
        const hipError_t e = hipMemsetAsync(W.ctr(), 0, kCtrTotal * sizeof(int), s);
        return e != hipSuccess ? e : hipMemsetAsync(W.s_zero(), 0, 32 * sizeof(double), s);
    }

    // A panel's reconstruction finishes (modified LU, T, the band block's
    // signs) in the first workgroup of the read pass that follows it, which
    // uses V' = Q; the last LQ panel of a block finishes inline (the block
    // update reads its U straight away).
    FinArgs fin(QtSrc q, double *sgn, T *tout, T *apan, long asi, long ast) const {
        return FinArgs{q.qt, q.zero, sgn, tout, apan, asi, ast};
    }

    // k_prep of panel (c, j) over `items` rows (QR) / columns (LQ), reading
    // the read pass's ks partials and G from the workspace; cc: PrepArgs::cc
    PrepArgs prep(int c, int j, int items, long cc, int ks, const T *Tm, const double *sgn) const {
        PrepArgs p;
        p.A = A; p.lda = lda; p.Lw = W.Lw(); p.RwT = W.RwT(); p.ldr = W.L.ldr;
        p.part = W.part(); p.mp = W.L.mp; p.ksplit = ks;
        p.G = W.vout(); p.Tm = Tm;
        p.Qp = W.Qp(); p.mq = W.L.mp;
        p.c = c; p.j = j; p.items = items; p.reduce = 0; p.factor = 0;
        p.sgn = sgn;
        p.cc = cc; p.zfill = 0;
        return p;
    }
    // the panel QR's first Gram partials formed by the prep kernel that writes
    // the panel (no k_cqr_gram launch; BRD_PREP_GRAM)
    void gram_into(PrepArgs &p) const {
        p.gram = 1;
        p.gpp = W.gpp();   // records [wg][kGramRec]
        p.gout = W.cqr().gp1; p.gew = W.cqr().ew; p.gcnt = W.ctr(kCtrGram);
    }
    hipError_t run_prep(bool lq, const PrepArgs &p) const { launch_k_prep<T>(lq, p, lc, s); return hipGetLastError(); }

    RpCall y_pass(int c, int j, long col, int ncols, const FinArgs *fq) const {
        RpCall r; r.yp = true;
        r.src = a(c, col); r.ld = lda; r.K = mrows - c; r.M = ncols;
        r.bsrc = W.V(c, j); r.bld = kLwCols;
        r.vsrc = W.Lw(c); r.vld = kLwCols;
        r.fin = fq;
        r.pbase = W.V(c, j); r.pstride = kLwCols + 1; r.psgn = W.s_q(j);
        return r;
    }
    RpCall x_pass(int c, long col, int ncols) const {
        RpCall r; r.yp = false;
        r.src = a(c + 32, col); r.ld = lda; r.K = ncols; r.M = mrows - c - 32;
        r.bsrc = W.Ub(col); r.bld = 32;
        r.vsrc = W.RwT(col); r.vld = W.L.ldr;
        return r;
    }
    hipError_t rpass(const RpCall &r, int *ksplit, bool *folded = nullptr) const {
        const bool dma = lc.rpass_dma && r.K > 0 &&
                         rpass_dma_ok(r.yp, r.K, r.M, sizeof(T), r.src, r.ld, r.vsrc, r.vld, r.bsrc, r.bld);
        const RpPlan pl = rpass_plan(dma, r.K, r.M, r.vsrc != nullptr, sizeof(T), kKsMax, lc);
        RpArgs a;
        a.src = r.src; a.ld = r.ld; a.vsrc = r.vsrc; a.vld = r.vld; a.bsrc = r.bsrc; a.bld = r.bld;
        a.K = r.K; a.M = r.M; a.va = r.va; a.vb = r.vb;
        a.mtiles = pl.mtiles; a.ksplit = pl.ksplit; a.kper = pl.kper;
        a.tiles = pl.tiles; a.ns = pl.ns; a.wst = pl.wst; a.nvirt = pl.nvirt;
        a.part = W.part(); a.mp = W.L.mp; a.vpart = W.vpart(); a.vout = r.vout ? r.vout : W.vout();
        a.counter = W.ctr(kCtrRpass); a.err = err; a.has_fin = r.fin ? 1 : 0;
        // the virtual tile's partials summed inside k_rpass_d when the caller's
        // consumers patch V's / U's top block themselves (may_fold) -- beside
        // other work only, where one fewer launch per pass is worth more than the
        // pass's longer tail; bitwise the same band either
        // way.  BRD_VSUM_FOLD=0 / 1 forces it.
        a.vfold = (r.may_fold && lc.vsum_fold && a.wst > 0 && a.nvirt > 0) ? 1 : 0;
        *ksplit = pl.ksplit;
        if (folded) *folded = a.vfold != 0;
        // algorithmic: the K x M source read once, 2 x 32 flops per element
        const double fl = 2.0 * 32 * r.K * r.M, by = (double)r.K * r.M * sizeof(T);
        launch_k_rpass<T>(r.yp, dim3(a.has_fin + pl.grid), a, r.fin ? *r.fin : FinArgs{}, s, fl, by);
        if (a.nvirt > 0 && !a.vfold)
            launch_k_vsum<T>((const T *)a.vpart, (T *)a.vout, a.nvirt, (T *)r.pbase, r.pstride, r.psgn, s);
        return hipGetLastError();
    }

    // One panel QR of M rows, the whole of it here (the sharded row panel changes that)
    CqrArgs cqr_args(int M) const {
        CqrArgs a;
        a.rec = nullptr; a.nrec = 1; a.rme = 0; a.rctr = nullptr;
        a.M = M; a.Mg = M; a.goff = 0; a.top = 1;
        a.vdst2 = nullptr; a.vsi2 = 0; a.vst2 = 0;
        a.ws = W.cqr().gp1; a.err = err; a.azero = 1; a.qcopy = nullptr;
        return a;
    }
    // the column panel (c, j), its first column at (local) col: from A (j = 0) or the corrected panel Qp
    CqrArgs qr_panel(int c, int j, long col) const {
        CqrArgs q = cqr_args(mrows - c);
        if (j == 0) { q.src = a(c, col); q.si = lda; q.st = 1; }
        else        { q.src = W.Qp(); q.si = 1; q.st = W.L.mp; }
        q.vdst = W.V(c, j); q.vsi = kLwCols; q.vst = 1;
        q.tout = W.Tf(j); q.apan = a(c, col); q.asi = lda; q.ast = 1;
        return q;
    }
    // the row panel of (c, j): ncols (local) columns from col, from Qp; U_j into RwT and Ub
    CqrArgs lq_panel(int c, int j, long col, int ncols) const {
        CqrArgs l = cqr_args(ncols);
        l.src = W.Qp(); l.si = 1; l.st = W.L.mp;
        l.vdst = W.U(j, col); l.vsi = 1; l.vst = W.L.ldr;
        l.vdst2 = W.Ub(col); l.vsi2 = 32; l.vst2 = 1;
        l.tout = W.Sf(j); l.apan = a(c, col); l.asi = 1; l.ast = lda;
        return l;
    }
    // inl: finish the reconstruction inline; gram_done: the prep kernel formed gp1 / ew
    hipError_t cqr(const CqrArgs &a, const FinArgs &f, bool inl, bool gram_done) const {
        const int nwg = (a.M + kCT - 1) / kCT;
        if (nwg > kCW) return hipErrorInvalidValue;
        if (!gram_done) launch_k_cqr<T>(kCqrGram, nwg, a, f, s);
        launch_k_cqr<T>(kCqrQ1, nwg, a, f, s);
        launch_k_cqr<T>(inl ? kCqrVInline : kCqrV, nwg, a, f, s);
        return hipGetLastError();
    }

    // the rank-256 update of the trailing matrix from row k1, `cols` (local)
    // columns from col
    hipError_t update(int k1, long col, int cols) const {
        GemmArgs g;
        g.C = a(k1, col); g.ldc = lda;
        g.rows = mrows - k1; g.cols = cols;
        g.Lw = W.Lw(k1); g.RwT = W.RwT(col); g.ldr = W.L.ldr; g.K = kLwCols;
        g.tiles_c = (g.cols + kGM - 1) / kGM;
        g.ntiles = ((g.rows + kGM - 1) / kGM) * g.tiles_c;
        // algorithmic: C read and written once, Lw / RwT read once; 2 x 256 flops per element
        const double el = (double)g.rows * g.cols;
        launch_k_blkupd<T>(g, lc, s, 2.0 * kLwCols * el, (2.0 * el + (double)kLwCols * (g.rows + g.cols)) * sizeof(T));
        return hipGetLastError();
    }
};

#define BLK_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

// Blocked stage 1 over columns [0, kend) (kend = blk_columns(m, n, 32) > 0);
// the caller finishes the remaining panels with the per-panel path.
template <typename T>
hipError_t blk_ge2band(T *A, int m, int n, long lda, void *wsv, hipStream_t s, int target, int *err) {
    const BlkWs<T> W(wsv, blk_layout(m, n, sizeof(T)));
    const BlkCall<T> C{A, lda, W, s1_launch(m, n, target), s, err, m};
    const int kend = blk_columns(m, n, 32);
    BLK_HIP(C.reset());
    int ks_x = 1;
    bool x_patch = false;                  // the previous X pass left U's top block for prep_qr to patch
    const double *sg_prev = W.s_zero();    // s of the previous LQ panel (prep_qr's correction)
    // the prep kernels form the next panel QR's first Gram partials (no
    // k_cqr_gram launch) unless BRD_PREP_GRAM says otherwise (A/B)
    const bool fold_qr = C.lc.prep_gram & 1, fold_lq = C.lc.prep_gram & 2;
    for (int k0 = 0; k0 < kend; k0 += NBMAX * 32) {
        for (int j = 0; j < NBMAX; ++j) {
            const int c = k0 + 32 * j;
            const int mr = m - c;          // rows of the column panel
            const int n2 = n - c - 32;     // columns right of it
            // ---- QR of the column panel -> V_j, T_j ------------------------------
            const FinArgs fq = C.fin(W.cqr_qt(), W.s_q(j), W.Tf(j), C.a(c, c), lda, 1);
            if (j > 0) {   // X_{j-1} and the corrected column panel
                PrepArgs p = C.prep(c, j, mr, c, ks_x, W.Sf(j - 1), sg_prev);
                p.reduce = 1; p.factor = 1;
                p.upatch = x_patch ? 1 : 0;
                if (fold_qr) C.gram_into(p);
                BLK_HIP(C.run_prep(false, p));
            }
            BLK_HIP(C.cqr(C.qr_panel(c, j, c), fq, false, j > 0 && fold_qr));
            // ---- Y pass (+ the QR panel's finish), the corrected row panel ----------
            int ks_y = 1;
            bool yfold = false, xfold = false;
            RpCall ry = C.y_pass(c, j, c + 32, n2, &fq);
            ry.may_fold = true; ry.va = 32 * j; ry.vb = 32 * j;
            BLK_HIP(C.rpass(ry, &ks_y, &yfold));
            {
                PrepArgs p = C.prep(c, j, n2, c + 32, ks_y, W.Tf(j), W.s_q(j));
                p.vpatch = yfold ? 1 : 0;
                if (fold_lq) C.gram_into(p);
                BLK_HIP(C.run_prep(true, p));
            }
            // ---- LQ of the row panel -> U_j, S_j ---------------------------------
            const bool inl = j == NBMAX - 1;
            const FinArgs fl = C.fin(W.cqr_qt(), W.s_l(j), W.Sf(j), C.a(c, c + 32), 1, lda);
            BLK_HIP(C.cqr(C.lq_panel(c, j, c + 32, n2), fl, inl, fold_lq));
            // ---- X pass (+ the LQ panel's finish) --------------------------------
            RpCall rx = C.x_pass(c, c + 32, n2);
            rx.psgn = W.s_l(j);
            if (!inl) { rx.fin = &fl; rx.pbase = W.U(j, c + 32); rx.pstride = W.L.ldr + 1; }
            rx.may_fold = true; rx.va = 32 * (j + 1); rx.vb = 32 * j;   // prep_qr(j + 1) / the block end read these
            BLK_HIP(C.rpass(rx, &ks_x, &xfold));
            x_patch = !inl && xfold;   // prep_qr of the next panel patches U_j's top block
            sg_prev = inl ? W.s_zero() : W.s_l(j);
        }
        // ---- block end: X_3, then the rank-256 update ---------------------------
        const int k1 = k0 + NBMAX * 32;
        PrepArgs p = C.prep(k1, NBMAX, m - k1, k1, ks_x, W.Sf(NBMAX - 1), sg_prev);   // sg_prev: the block's last
        p.reduce = 1;                                                                // LQ panel finished inline: zeros
        BLK_HIP(C.run_prep(false, p));
        BLK_HIP(C.update(k1, k1, n - k1));
    }
    return hipSuccess;
}

template hipError_t blk_ge2band<double>(double *, int, int, long, void *, hipStream_t, int, int *);
template hipError_t blk_ge2band<float>(float *, int, int, long, void *, hipStream_t, int, int *);

// ==========================================================================
// The blocked path sharded over P GPUs (brd_dist.hip's layout: global column
// panel p on rank p mod P; DESIGN.md "Multi-GPU" has the steps in full).  Lw =
// [V | X] (m x 256) is replicated, RwT = [Y | U] and Ub hold this rank's
// columns; the block update is local to each rank's columns.  Per panel j
// (global panel p, column c), five collectives:
//   QR   the owner of panel p forms the corrected column panel (k_prep_qr,
//        after every rank has added X_{j-1} to its Lw from the all-reduced X
//        partials) and runs its CholeskyQR; V' = Q (m - c rows), Q_t and the
//        zero flag are BROADCAST; every rank finishes the reconstruction
//        (modified LU, T_j, signs) beside its own Y pass, which is local.
//   LQ   every rank corrects its columns of the row panel (k_prep_lq) and
//        factors its rows of the panel's transpose by a SHARDED CholeskyQR:
//        per pass a local 32 x 32 Gram (the kernel's last workgroup sums its
//        partials into this rank's record), an ALL-GATHER of the P records
//        (8 KB each), summed in rank order by every rank -- the same R on
//        every rank, bit for bit -- and the local Q = P R^-1; three
//        all-gathers per panel (G1, G2 and sCQR3's middle Gram).  The rank
//        holding panel p + 1 (the panel's top block) finishes the
//        reconstruction inline, S_j straight into its slot of the X
//        all-reduce (the other ranks zero it, so the sum is S_j exactly).
//   X    X_j = A U_j S_j sums over columns: each rank's split-K partials (and
//        its part of G = Rw^T U_j) are summed locally (k_dist_psum) and
//        ALL-REDUCED (m - c - 32 + 256 rows of 32, and S_j).
// With one rank every collective is the identity and the path is the one-GPU
// blk_ge2band, launch for launch.
// ==========================================================================
static int bd_fail(hipError_t e, int line) {
    char m_[256];
    snprintf(m_, sizeof m_, "blocked distributed stage 1: %s (%s:%d)", hipGetErrorString(e), __FILE__, line);
    return api_fail(BRD_EHIP, m_);
}
#define BD_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return bd_fail(e_, __LINE__); } while (0)
#define BD_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

template <typename T>
int blk_ge2band_dist(T *A, int m, int n, long lda, Comm &Cm, void *wsv, hipStream_t s, int target, int *err) {
    const int P = Cm.nranks, me = Cm.rank;
    if (P == 1) {
        // one rank: every collective below is the identity and every rank-local
        // piece is the whole panel -- the one-GPU blocked path is this path
        // (its workspace is the head of this one's), launch for launch
        BD_HIP(blk_ge2band<T>(A, m, n, lda, wsv, s, target, err));
        return BRD_OK;
    }
    const int n_loc = dist_local_cols(n, 32, P, me);
    const int kend = blk_columns(m, n, 32);
    const BlkWs<T> W(wsv, blk_layout(m, std::max(n_loc, 1), sizeof(T)), dist_blk_layout(m, n, P, me, sizeof(T)), P);
    const BlkCall<T> C{A, lda, W, s1_launch(m, n, target), s, err, m};
    const int dt = sizeof(T) == 8 ? BRD_DT_F64 : BRD_DT_F32;
    // every counter, the prep Gram groups' included: the workspace is shared
    // with the per-panel tail and the band gather, and a nonzero group counter
    // would hold back the last-arriver's Gram sum
    BD_HIP(C.reset());
    const T *s_prev = nullptr;   // S_{j-1}: the previous panel's all-reduced slot
    // X_{j-1} (j = NBMAX: X_3 at the block end) from the all-reduced sums
    auto prep_x = [&](int c, int j, long cc) {
        PrepArgs p = C.prep(c, j, m - c, cc, 1, s_prev, W.s_zero());
        p.part = W.ar_X(); p.mp = 0; p.G = W.ar_G();
        p.reduce = 1;
        return p;
    };
    for (int k0 = 0; k0 < kend; k0 += NBMAX * 32) {
        for (int j = 0; j < NBMAX; ++j) {
            const int p = k0 / 32 + j, c = 32 * p, mr = m - c, mx = m - c - 32;
            const int o = p % P, o2 = (p + 1) % P;          // owners of panel p and of panel p + 1
            const bool own = me == o, own2 = me == o2;
            const long lco = (long)(p / P) * 32;            // panel p's column on its owner
            const long lcs = (long)dist_panels_before(p + 1, P, me) * 32;   // first local trailing column
            const int nc = n_loc - (int)lcs;                 // local trailing columns
            // ---- X_{j-1} (every rank) + the column panel's QR (its owner) ----------
            const bool fold_qr = own && j > 0 && (C.lc.prep_gram & 1);
            if (j > 0) {
                PrepArgs pa = prep_x(c, j, lco);
                pa.factor = own ? 1 : 0;
                if (fold_qr) C.gram_into(pa);
                BD_HIP(C.run_prep(false, pa));
            }
            const QtSrc bq = W.bc_qt(mr);
            const FinArgs fq = C.fin(bq, W.s_q(j), W.Tf(j), own ? C.a(c, lco) : nullptr, lda, 1);
            if (own) {
                CqrArgs q = C.qr_panel(c, j, lco);
                q.vdst2 = W.bc_v(); q.vsi2 = 32; q.vst2 = 1;   // V' and Q_t + flag into the broadcast buffer
                q.qcopy = bq.qt;
                BD_HIP(C.cqr(q, fq, false, fold_qr));
            }
            BD_TRY(Cm.bcast(W.bc_v(), W.bc_bytes(mr), o, s));
            if (!own) launch_dist_unpack_v<T>(W.bc_v(), W.V(c, j), mr, s);
            // ---- Y pass (local columns; every rank finishes the QR panel) -----------
            int ks_y = 1;
            BD_HIP(C.rpass(C.y_pass(c, j, lcs, nc, &fq), &ks_y));
            // ---- the row panel: corrected locally, factored by a sharded CholeskyQR --
            BD_HIP(C.run_prep(true, C.prep(c, j, nc, lcs, ks_y, W.Tf(j), W.s_q(j))));
            T *sj_ar = W.ar_S(mx);   // S_j's slot at the tail of the X all-reduce
            {
                CqrArgs a = C.lq_panel(c, j, lcs, std::max(nc, 0));
                a.rec = W.rec(0); a.nrec = P; a.rme = me; a.rctr = W.ctr(kCtrDistQr);
                a.Mg = n - c - 32;
                a.goff = (long)((me - o2 + P) % P) * kCW * kCT;
                a.top = own2 ? 1 : 0;
                const int nwg = std::max(1, (a.M + kCT - 1) / kCT);
                // S_j straight into its slot of the X all-reduce (the other
                // ranks add exact zeros: the sum is S_j bit for bit), which
                // replaces a broadcast of its own
                const FinArgs fl = C.fin(W.cqr_qt(), W.s_l(j), own2 ? sj_ar : W.Sf(j), own2 ? C.a(c, lcs) : nullptr, 1, lda);
                if (!own2) BD_HIP(hipMemsetAsync(sj_ar, 0, kQt * sizeof(T), s));
                const size_t rb = (size_t)kCqrRec * sizeof(double);
                launch_k_cqr<T>(kCqrGram, nwg, a, fl, s);   // -> record bank 0: this rank's G1, exponent
                BD_TRY(Cm.allgather(W.rec(0, me), W.rec(0), rb, s));
                launch_k_cqr<T>(kCqrQ1, nwg, a, fl, s);     // R1 (every rank, the same), Q1 rows -> bank 1
                BD_TRY(Cm.allgather(W.rec(1, me), W.rec(1), rb, s));
                launch_k_cqr<T>(kCqrMid, nwg, a, fl, s);    // sCQR3's middle pass (shifted panels) -> bank 2
                BD_TRY(Cm.allgather(W.rec(2, me), W.rec(2), rb, s));
                // V rows into RwT and Ub; the top block's owner finishes inline (LU, S_j, the band block)
                launch_k_cqr<T>(own2 ? kCqrVInline : kCqrV, nwg, a, fl, s);
                BD_HIP(hipGetLastError());
            }
            // ---- X pass (local columns), partials summed and all-reduced ------------
            if (nc > 0) {
                int ks_x = 1;
                RpCall rx = C.x_pass(c, lcs, nc);
                rx.vout = W.ar_G();
                BD_HIP(C.rpass(rx, &ks_x));
                launch_dist_psum<T>((const T *)W.part(), ks_x, W.L.mp, mx, W.ar_X(), s);
            } else {
                BD_HIP(hipMemsetAsync(W.ar_G(), 0, W.ar_gx_count(mx) * sizeof(T), s));
            }
            BD_TRY(Cm.allreduce_sum(W.ar_G(), W.ar_count(mx), dt, s));
            s_prev = sj_ar;   // read by the next prep_qr / the block end, before the next X pass writes ar
        }
        // ---- block end: X_3 (every rank), the rank-256 update of my columns ---------
        const int k1 = k0 + NBMAX * 32;
        BD_HIP(C.run_prep(false, prep_x(k1, NBMAX, 0)));
        const long lck = (long)dist_panels_before(k1 / 32, P, me) * 32;
        if (n_loc - (int)lck > 0) BD_HIP(C.update(k1, lck, n_loc - (int)lck));
    }
    return BRD_OK;
}
template int blk_ge2band_dist<double>(double *, int, int, long, Comm &, void *, hipStream_t, int, int *);
template int blk_ge2band_dist<float>(float *, int, int, long, Comm &, void *, hipStream_t, int, int *);

}  // namespace brd
