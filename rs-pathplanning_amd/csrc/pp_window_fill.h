// pp_window_fill.h — which iterations a window takes: K bounds the samples a window SCREENS, not
// the iterations it spans.  Plain C++ (no HIP header): samples_role uses it on the device, the
// tests compile it with the host compiler.
//
// A draw whose point lies in an obstacle (the pre-test) is rejected whatever the tree looks like:
// it is settled where it is drawn and takes no sample id, so it costs the window nothing.  The
// window starting at iteration `start` therefore draws iterations start, start + 1, ... and gives
// the live draws the ids 0, 1, ... in iteration order, until it holds Kw of them:
//   cap   C = min(2 Kw, target - start)   the most iterations a window may span (the draws are
//                                         bounded, however many are blocked); pre-test off: Kw
//   span    = the offset of the (Kw + 1)-th live draw, or C when fewer than Kw + 1 draws are live
//   W       = the live draws in [0, span)  (<= Kw)
// The next window starts at start + span, so consecutive windows tile the iterations.  The draws
// are made in rounds and stop with the round that decides the span (samples_role: 4096 draws, four
// per thread, then 2048 at a time; a window of Kw <= 2048 is one round).
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define PP_FILL_FN __attribute__((host)) __attribute__((device)) inline
#else
#define PP_FILL_FN inline
#endif

namespace ppamd {

struct WindowFill {
    int W;     // live samples: ids 0 .. W - 1
    int span;  // iterations the window covers
};

// the most iterations the window at `start` may span (rem = target - start)
PP_FILL_FN int window_fill_cap(int Kw, int64_t rem, bool pretest) {
    if (rem <= 0 || Kw <= 0) return 0;
    const int64_t c = pretest ? 2 * (int64_t)Kw : (int64_t)Kw;
    return (int)(rem < c ? rem : c);
}

// the draws go on while the span is undecided: fewer than Kw + 1 live draws, and draws left
PP_FILL_FN bool window_fill_more(int Kw, int cap, int drawn, int live) {
    return drawn < cap && live <= Kw;
}

// the end of the round that starts at draw `drawn`: `first` draws in the first round, `later` in
// every other
PP_FILL_FN int window_fill_round_end(int cap, int drawn, int first, int later) {
    const int64_t e = (int64_t)drawn + (drawn == 0 ? first : later);
    return (int)(e < cap ? e : cap);
}

// the window, from the live draws counted (all of them when fewer than Kw + 1 were found, else at
// least Kw + 1) and the offset of the (Kw + 1)-th (only read when there is one)
PP_FILL_FN WindowFill window_fill_close(int Kw, int cap, int live, int off_next) {
    WindowFill f;
    if (live > Kw) {
        f.W = Kw;
        f.span = off_next;
    } else {
        f.W = live;
        f.span = cap;
    }
    return f;
}

// One window, one draw at a time (the host's sweep; the device runs the same rounds with a
// workgroup): blocked(i) tells whether draw i of the window lies in an obstacle, iter_off[id]
// receives the offset of live sample id (Kw entries at most).  drawn (optional): the draws made.
template <typename Blocked>
PP_FILL_FN WindowFill window_fill_seq(int Kw, int64_t rem, bool pretest, int first, int later,
                                      Blocked blocked, int* iter_off, int* drawn_out = nullptr) {
    const int cap = window_fill_cap(Kw, rem, pretest);
    int drawn = 0, live = 0, off_next = -1;
    while (window_fill_more(Kw, cap, drawn, live)) {
        const int end = window_fill_round_end(cap, drawn, first, later);
        for (int i = drawn; i < end; ++i) {
            if (pretest && blocked(i)) continue;
            if (live < Kw)
                iter_off[live] = i;
            else if (live == Kw)
                off_next = i;
            ++live;
        }
        drawn = end;
    }
    if (drawn_out) *drawn_out = drawn;
    return window_fill_close(Kw, cap, live, off_next);
}

}  // namespace ppamd
