// pp_screen_geom.h — the tiling of the NN screen: which workgroup screens which samples against
// which tree nodes.  Plain C++ (no HIP header): samples_role, the screen and nn_finalize use it on
// the device, the tests compile it with the host compiler.
//
// The screened samples (sorted positions [0, Ws)) are rows of 64, one sample per lane.  A sample
// block is 1..8 consecutive rows (a lane's accumulators); its workgroups split the tree's nodes
// into the block's own number of chunks.  The rows are split as evenly as they go over
// ceil(rows / 8) blocks and every block gets chunks in proportion to its rows, so each of the (at
// most kScanGrid) workgroups has about the same rows x nodes to do.
#pragma once

#if defined(__HIP__)
#define PP_GEOM_FN __attribute__((host)) __attribute__((device)) constexpr
#else
#define PP_GEOM_FN constexpr
#endif

namespace ppamd {

constexpr int kMaxChunks = 64;     // node chunks of a sample block (partials per sample)
constexpr int kScanGrid = 255;     // screen workgroups per window (one per CU, with the resolve
                                   // workgroup: <= 256 CUs)
constexpr int kScanWaves = 8;      // waves of a screen workgroup (they split its chunk)
constexpr int kScanBlk = 16;       // nodes per block (one block minimum per sample)
constexpr int kQPL = 8;            // rows of a sample block at most (samples per lane)
constexpr int kQPB = 64 * kQPL;    // samples of a full block
constexpr int kScreenBlocks = 8;   // sample blocks at most (kMaxWindow / kQPB)

struct ScreenTile {
    short row0 = 0, rows = 0;  // the block's rows [row0, row0 + rows): sorted positions 64 row0 ...
    short chunks = 0;          // its node chunks (<= kMaxChunks)
    short wg0 = 0;             // workgroups of the blocks before it
};
struct ScreenGeom {
    int nb = 0;  // sample blocks
    int G = 0;   // workgroups: the sum of the blocks' chunks (<= kScanGrid)
    ScreenTile t[kScreenBlocks] = {};
};

// nodes per chunk when n nodes go over `chunks` chunks: whole blocks, and at least one block per
// wave of the workgroup (fewer chunks are used then: screen_chunks_used)
PP_GEOM_FN int scan_chunk_len(int n, int chunks) {
    int cl = (n + chunks - 1) / chunks;
    if (cl < kScanWaves * kScanBlk) cl = kScanWaves * kScanBlk;
    return (cl + kScanBlk - 1) & ~(kScanBlk - 1);
}
PP_GEOM_FN int scan_chunks_used(int n, int chunks) {
    const int cl = scan_chunk_len(n, chunks);
    return (n + cl - 1) / cl;
}

// Rows split evenly over nb blocks: base = R / nb rows each, the first extra = R % nb one more.
// Block k's first row:
PP_GEOM_FN int screen_split_row0(int base, int extra, int k) {
    return k * base + (k < extra ? k : extra);
}
// ... and the block of a row (branch-free; rows past the last block's start stay in it)
PP_GEOM_FN int screen_split_block(int base, int extra, int nb, int row) {
    int k = 0;
    for (int j = 1; j < kScreenBlocks; ++j)
        k += (j < nb && row >= screen_split_row0(base, extra, j)) ? 1 : 0;
    return k;
}

// The tiling for Ws screened samples.  It does not depend on the tree: a block's chunk length
// follows from its chunk count and the nodes at hand (scan_chunk_len).
PP_GEOM_FN void screen_geom(int Ws, ScreenGeom* g) {
    const int R = Ws > 0 ? (Ws + 63) / 64 : 0;
    const int nb = (R + kQPL - 1) / kQPL;
    g->nb = nb;
    g->G = 0;
    for (int k = 0; k < kScreenBlocks; ++k) g->t[k] = ScreenTile{0, 0, 0, 0};  // (constexpr: all set)
    if (nb == 0) return;
    const int base = R / nb, extra = R % nb;  // the first `extra` blocks take one row more
    int sum = 0;
    for (int k = 0; k < nb; ++k) {
        const int row = screen_split_row0(base, extra, k);
        const int rows = screen_split_row0(base, extra, k + 1) - row;
        int c = rows * kScanGrid / R;
        if (c > kMaxChunks) c = kMaxChunks;
        g->t[k].row0 = (short)row;
        g->t[k].rows = (short)rows;
        g->t[k].chunks = (short)c;
        sum += c;
    }
    // the workgroups the rounding left over go where the rows per chunk are highest
    for (int left = kScanGrid - sum; left > 0; --left) {
        int m = -1;
        for (int k = 0; k < nb; ++k) {
            if (g->t[k].chunks >= kMaxChunks) continue;
            if (m < 0 || g->t[k].rows * g->t[m].chunks > g->t[m].rows * g->t[k].chunks) m = k;
        }
        if (m < 0) break;
        ++g->t[m].chunks;
    }
    sum = 0;
    for (int k = 0; k < nb; ++k) {
        g->t[k].wg0 = (short)sum;
        sum += g->t[k].chunks;
    }
    g->G = sum;
}

// the block that holds row `row` (a sorted position's row is position / 64), and its chunks.
// Branch-free over all the entries: on the device the tiles are one wide load, not a chain.
PP_GEOM_FN int screen_block_of_row(const ScreenGeom& g, int row) {
    int k = 0;
    for (int j = 1; j < kScreenBlocks; ++j) k += (j < g.nb && row >= g.t[j].row0) ? 1 : 0;
    return k;
}
PP_GEOM_FN int screen_chunks_of_row(const ScreenGeom& g, int row) {
    int c = g.t[0].chunks;
    for (int j = 1; j < kScreenBlocks; ++j) c = (j < g.nb && row >= g.t[j].row0) ? g.t[j].chunks : c;
    return c;
}

// The work list: every (block k, chunk c), ordered by the chunk's place in the tree, c / chunks_k
// (then k) — neighbours in the list stream neighbouring node ranges.  This is (k, c)'s position.
PP_GEOM_FN int screen_work_rank(const ScreenGeom& g, int k, int c) {
    const int ck = g.t[k].chunks;
    int r = c;
    for (int j = 0; j < g.nb; ++j) {
        const int cj = g.t[j].chunks;
        if (j < k) r += c * cj / ck + 1;              // c' / cj <= c / ck
        if (j > k) r += (c * cj + ck - 1) / ck;       // c' / cj <  c / ck
    }
    return r;
}

// Workgroup b of G (dispatched round-robin over the 8 XCDs) takes this position of the work list:
// XCD b % 8 gets a contiguous range, so the workgroups that stream one node range share an L2.
PP_GEOM_FN int screen_xcd_slot(int G, int b) {
    const int x = b & 7, q = G >> 3, r = G & 7;
    return x * q + (x < r ? x : r) + (b >> 3);
}

// The tiling depends on the screened samples only through their rows, ceil(Ws / 64) = 0..64: both
// tables are built at compile time and the screen and nn_finalize look them up (computed by one
// thread of samples_role the tiling cost the sampling workgroup 3.8 us; samples_role itself
// needs only the row split, which is arithmetic).
constexpr int kScreenRowsMax = kScreenBlocks * kQPL;
// a workgroup's tile in one word: chunk c | block k << 6 | rows << 9 | row0 << 13 | chunks << 19
// (0: the workgroup is idle), so a screen workgroup learns its tile from one load
struct ScreenWork {
    int k, c, rows, row0, chunks;
};
PP_GEOM_FN unsigned screen_work_pack(const ScreenGeom& g, int k, int c) {
    return (unsigned)c | (unsigned)k << 6 | (unsigned)g.t[k].rows << 9 |
           (unsigned)g.t[k].row0 << 13 | (unsigned)g.t[k].chunks << 19;
}
PP_GEOM_FN ScreenWork screen_work_unpack(unsigned e) {
    return ScreenWork{(int)(e >> 6 & 7), (int)(e & 63), (int)(e >> 9 & 15), (int)(e >> 13 & 63),
                      (int)(e >> 19 & 127)};
}
struct ScreenTables {
    ScreenGeom g[kScreenRowsMax + 1] = {};      // by rows
    unsigned wg[kScreenRowsMax + 1][256] = {};  // by rows and workgroup b: its tile, packed
};
constexpr ScreenTables make_screen_tables() {
    ScreenTables T;
    for (int R = 0; R <= kScreenRowsMax; ++R) {
        ScreenGeom& g = T.g[R];
        screen_geom(64 * R, &g);
        unsigned wl[256] = {};  // the work list: position -> tile
        for (int k = 0; k < g.nb; ++k)
            for (int c = 0; c < g.t[k].chunks; ++c)
                wl[screen_work_rank(g, k, c)] = screen_work_pack(g, k, c);
        for (int b = 0; b < g.G; ++b) T.wg[R][b] = wl[screen_xcd_slot(g.G, b)];
    }
    return T;
}
// (the kernels' unit keeps its own copy in constant memory)
PP_GEOM_FN int screen_rows(int Ws) { return Ws > 0 ? (Ws + 63) / 64 : 0; }

}  // namespace ppamd
