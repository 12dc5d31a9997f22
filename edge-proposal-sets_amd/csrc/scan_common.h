// What the one-pass scan's translation units share, each thing defined once: scan_pieces.hip (the piece kernel, its planner and
// the launch), scan_tables.hip (the per-graph and per-weight-table builders) and scan_heads.hip (skipped heads -- the head table,
// the hub adjacency bitmaps, the completion of the walked sums).  The layouts of the tables the builders write and the piece kernel reads (cuts, row records, plan records, the
// column pack) are told where sp_params names them, in scan_pieces.hip.
#pragma once
#include "eps_common.h"

#define SP_M 32                 // id windows per graph (one 64-byte row of cuts per node); 48 windows: 1.99 M instead of 2.03 M pieces, -0.5 % (r04)
#define SP_FLAG 0x80000000u      // value word of a KNOWN EDGE's endpoint (put in before the walk): sums stay below 2^31, so the bit survives them
                                 // (not in sketch pieces: they put no flags in, their estimates may reach 2^32 - 1 and are compared unsigned)

#if defined(__HIPCC__)
// The bar in the table's domain.  filter_scan.hip keeps a candidate when its 2^-40 fixed-point sum a satisfies
// float(a * 2^-40) > threshold, i.e. a >= thr_fix (monotone: found by bisection); a screening sum s >= a / 2^(40 - shift),
// so s >= floor(thr_fix / 2^(40 - shift)) holds for every such candidate.  Any bar <= 0 (or -inf): every candidate (1).
// +inf / NaN: nothing passes (SP_FLAG: sums stay below 2^31).
// ``up``: the quotient rounded UP instead -- s is a whole number, so s >= ceil(thr_fix / 2^(40 - shift)) holds for every such
// candidate just as well, and then float(s * 2^-shift) >= float(thr_fix * 2^-40) > threshold: every reported screening score
// exceeds the bar.  The launches over stored values take it (their list goes straight to the re-scoring); the unit-valued ones
// keep the floor, which eps_scan_refine shares with them (a walked sum AT the bar in table units passes there).
__device__ __forceinline__ uint32_t sp_bar_units(float thr, int shift, bool up = false)
{
    auto above = [&](long long a) { return (float)((double)a * (1.0 / (double)(1ll << 40))) > thr; };
    if (!above(0x7fffffffffffffffll)) return SP_FLAG;
    if (above(0ll)) return 1u;
    long long lo = 1ll, hi = 0x7fffffffffffffffll;      // smallest positive a with above(a)
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (above(mid)) hi = mid; else lo = mid + 1;
    }
    const unsigned long long q = ((unsigned long long)lo + (up ? (1ull << (40 - shift)) - 1ull : 0ull)) >> (40 - shift);
    return q >= (unsigned long long)SP_FLAG ? SP_FLAG : (q ? (uint32_t)q : 1u);
}
#endif
