// Sweeps the NN screen's tiling (rs-pathplanning_amd/csrc/pp_screen_geom.h) on the host: every
// Ws in 0..4096 against a list of tree sizes.  Prints one JSON line; exits 1 with the first
// violated property on stderr.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pp_screen_geom.h"

using namespace ppamd;

#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            std::fprintf(stderr, "Ws=%d ns=%d: ", Ws, ns);      \
            std::fprintf(stderr, __VA_ARGS__);                  \
            std::fprintf(stderr, " (%s)\n", #cond);             \
            return 1;                                           \
        }                                                       \
    } while (0)

// the tables the kernels look up, built at compile time as in the kernels' unit
static constexpr ScreenTables T = make_screen_tables();

int main() {
    const int sizes[] = {0, 1, 15, 16, 127, 128, 129, 1000, 7936, 7937, 65536, 100000, 250000};
    double worst = 0.0;
    int worst_ws = 0, worst_ns = 0;
    long pairs = 0;
    for (int Ws = 0; Ws <= 4096; ++Ws) {
        const int R = (Ws + 63) / 64;
        ScreenGeom g;
        screen_geom(Ws, &g);
        {  // the table entry of Ws's rows is the tiling of Ws
            const int ns = -1;
            const ScreenGeom& t = T.g[screen_rows(Ws)];
            CHECK(screen_rows(Ws) == R && t.nb == g.nb && t.G == g.G, "table entry %d", R);
            for (int k = 0; k < kScreenBlocks; ++k)
                CHECK(t.t[k].row0 == g.t[k].row0 && t.t[k].rows == g.t[k].rows &&
                          t.t[k].chunks == g.t[k].chunks && t.t[k].wg0 == g.t[k].wg0,
                      "table entry %d block %d", R, k);
        }
        for (int ns : sizes) {
            ++pairs;
            CHECK(g.nb == (R + 7) / 8, "blocks %d", g.nb);
            CHECK(g.G <= kScanGrid, "workgroups %d", g.G);
            // rows: each in exactly one block, 1..8 per block, split as evenly as they go
            std::vector<int> rowcov(R, 0);
            int sum = 0, rmin = 99, rmax = 0;
            for (int k = 0; k < g.nb; ++k) {
                const ScreenTile& t = g.t[k];
                CHECK(t.rows >= 1 && t.rows <= kQPL, "block %d rows %d", k, t.rows);
                CHECK(t.chunks >= 1 && t.chunks <= kMaxChunks, "block %d chunks %d", k, t.chunks);
                CHECK(t.wg0 == sum, "block %d wg0 %d", k, t.wg0);
                sum += t.chunks;
                rmin = t.rows < rmin ? t.rows : rmin;
                rmax = t.rows > rmax ? t.rows : rmax;
                CHECK(screen_split_row0(R / g.nb, R % g.nb, k) == t.row0, "block %d split row0", k);
                for (int r = t.row0; r < t.row0 + t.rows; ++r) {
                    CHECK(screen_split_block(R / g.nb, R % g.nb, g.nb, r) == k, "row %d split block", r);
                    CHECK(r >= 0 && r < R, "block %d row %d", k, r);
                    ++rowcov[r];
                    CHECK(screen_block_of_row(g, r) == k && screen_chunks_of_row(g, r) == t.chunks,
                          "row %d block lookup", r);
                }
                // chunks in proportion to the rows (within the rounding, and the cap)
                if (t.chunks < kMaxChunks) {
                    CHECK((t.chunks + 1) * R > t.rows * kScanGrid, "block %d chunks %d low", k, t.chunks);
                }
                // nodes: the used chunks tile [0, ns) once, whole blocks, one block per wave
                const int cl = scan_chunk_len(ns, t.chunks);
                const int used = scan_chunks_used(ns, t.chunks);
                CHECK(cl % kScanBlk == 0, "block %d chunk length %d", k, cl);
                CHECK(used <= t.chunks, "block %d uses %d of %d chunks", k, used, t.chunks);
                CHECK(used == 1 || cl >= kScanWaves * kScanBlk, "block %d chunk length %d", k, cl);
                long covered = 0;
                for (int c = 0; c < t.chunks; ++c) {
                    const long c0 = (long)c * cl;
                    if (c0 >= ns) {
                        CHECK(c >= used, "block %d chunk %d empty", k, c);
                        continue;
                    }
                    CHECK(c < used && c0 == covered, "block %d chunk %d starts at %ld", k, c, c0);
                    covered = c0 + cl < ns ? c0 + cl : ns;
                }
                CHECK(covered == ns, "block %d covers %ld nodes", k, covered);
                // balance: the largest workgroup against an even split over the grid
                if (Ws >= 2048 && ns >= 65536) {
                    const double ratio = (double)t.rows * cl / ((double)R * ns / kScanGrid);
                    if (ratio > worst) worst = ratio, worst_ws = Ws, worst_ns = ns;
                    CHECK(ratio <= 1.05, "block %d: %d rows x %d nodes is %.4f of the even split", k,
                          t.rows, cl, ratio);
                }
            }
            CHECK(sum == g.G, "workgroups %d, blocks' chunks %d", g.G, sum);
            CHECK(g.nb == 0 || rmax - rmin <= 1, "rows %d..%d per block", rmin, rmax);
            for (int r = 0; r < R; ++r) CHECK(rowcov[r] == 1, "row %d in %d blocks", r, rowcov[r]);
            // workgroup -> work list position -> (block, chunk): a bijection, each XCD a
            // contiguous range of the list
            std::vector<int> item(g.G, -1), slot(g.G, -1);
            for (int k = 0; k < g.nb; ++k)
                for (int c = 0; c < g.t[k].chunks; ++c) {
                    const int r = screen_work_rank(g, k, c);
                    CHECK(r >= 0 && r < g.G && item[r] < 0, "rank %d of (%d, %d)", r, k, c);
                    item[r] = k * 256 + c;
                }
            for (int r = 1; r < g.G; ++r) {  // ordered by c / chunks, then block
                const int k0 = item[r - 1] >> 8, c0 = item[r - 1] & 255, k1 = item[r] >> 8, c1 = item[r] & 255;
                const int a = c0 * g.t[k1].chunks, b = c1 * g.t[k0].chunks;
                CHECK(a < b || (a == b && k0 < k1), "work list order at %d", r);
            }
            int lo[8], hi[8];
            for (int x = 0; x < 8; ++x) lo[x] = 1 << 30, hi[x] = -1;
            for (int b = 0; b < g.G; ++b) {
                const int s = screen_xcd_slot(g.G, b);
                CHECK(s >= 0 && s < g.G && slot[s] < 0, "workgroup %d slot %d", b, s);
                slot[s] = b;
                const ScreenWork w = screen_work_unpack(T.wg[R][b]);  // the kernels' one-load form
                CHECK(w.k * 256 + w.c == item[s] && w.rows == g.t[w.k].rows &&
                          w.row0 == g.t[w.k].row0 && w.chunks == g.t[w.k].chunks,
                      "workgroup %d table entry", b);
                lo[b & 7] = s < lo[b & 7] ? s : lo[b & 7];
                hi[b & 7] = s > hi[b & 7] ? s : hi[b & 7];
            }
            for (int b = g.G; b < 256; ++b) CHECK(T.wg[R][b] == 0, "workgroup %d idle", b);
            for (int x = 0; x < 8 && x < g.G; ++x) {
                const int cnt = (g.G - x + 7) / 8;
                CHECK(hi[x] - lo[x] + 1 == cnt, "XCD %d: slots %d..%d for %d workgroups", x, lo[x], hi[x], cnt);
            }
        }
    }
    ScreenGeom a, b;
    screen_geom(2797, &a);
    screen_geom(4096, &b);
    std::printf("{\"pairs\": %ld, \"worst\": %.6f, \"worst_ws\": %d, \"worst_ns\": %d, \"g2797\": %d, "
                "\"g4096\": %d, \"rows2797\": [%d, %d, %d, %d, %d, %d], \"chunks2797\": [%d, %d, %d, %d, %d, %d]}\n",
                pairs, worst, worst_ws, worst_ns, a.G, b.G, a.t[0].rows, a.t[1].rows, a.t[2].rows,
                a.t[3].rows, a.t[4].rows, a.t[5].rows, a.t[0].chunks, a.t[1].chunks, a.t[2].chunks,
                a.t[3].chunks, a.t[4].chunks, a.t[5].chunks);
    return 0;
}
