// What the one-pass scan's translation units share, each thing defined once: scan_pieces.hip (the piece kernel, its planner and
// the launch), scan_light.hip (the lean kernel of light single-piece columns, launched by the same call), scan_tables.hip (the per-graph and per-weight-table builders) and scan_heads.hip (skipped heads -- the head table,
// the hub adjacency bitmaps, the completion of the walked sums).  The layouts of the tables the builders write and the piece kernel reads (cuts, row records, plan records, the
// column pack) are told where sp_params names them, in scan_pieces.hip.
#pragma once
#include "eps_common.h"

#define SP_M 32                 // id windows per graph (one 64-byte row of cuts per node); 48 windows: 1.99 M instead of 2.03 M pieces, -0.5 % (r04)
#define SP_FLAG 0x80000000u      // value word of a KNOWN EDGE's endpoint (put in before the walk): sums stay below 2^31, so the bit survives them
                                 // (not in sketch pieces: they put no flags in, their estimates may reach 2^32 - 1 and are compared unsigned)

#define SP_EM 128               // slots of the per-column set of ids a SKETCH piece has reported (a power of two; one per workgroup in the piece kernel, per wave in the light one)

#if defined(__HIPCC__)
struct sp_params {
    const int64_t *rowptr;
    const int32_t *col;
    const int32_t *revpos;
    const uint32_t *fx32;       // screening weight per node (>= 1); weighted graphs: unused
    const float *val;           // stored values A[.,.] (weighted graphs: HV) or NULL
    const float *node_w;        // float node weights (weighted graphs): a path's term is (A[u,w] * A[v,w]) * node_w[w]
    float up;                   // weighted graphs: 2^shift * (1 + 2^-20), the scale of the per-row factor
    const uint16_t *cuts;       // [n_nodes][SP_M]
    const uint32_t *wpaths;     // [n_nodes][SP_M] two-hop half paths of column v per id window (per-graph table) or NULL
    const int32_t *bounds;      // [SP_M + 1]
    const int32_t *columns;
    int32_t n_columns;
    int32_t n_nodes;
    uint32_t col_bytes;
    int32_t table_bits;         // slots = 1 << table_bits (keys) + as many values
    uint32_t piece_paths;       // a hash piece holds at most this many paths (<= slots / 2)
    const uint32_t *ssum;       // [n_nodes] sum of fx32 over the node's neighbours (an upper bound of any of its pairs' sums) or NULL
    const uint32_t *smax;       // [SP_M + 1] largest ssum among the ids >= bounds[k] (0 for k = SP_M); NULL with ssum
    uint32_t packed_paths;      // a PACKED hash piece holds at most this many paths (<= slots: key and sum share a word)
    int32_t packed_dmax;        // ... and may drop at most this many low bits of the screening weights
    const uint32_t *pptr;       // [n_nodes + 1] first plan record of column v (per-graph plan table) or NULL: the kernel plans itself
    const uint4 *plan;          // one record per piece: x = paths | kind bits, y = k0 | k1 << 8 | pq << 16, z = na | nb << 16, w = lo
    uint32_t mode_ratio;        // fixed cost of a piece in units of (a hashed path's cost - a direct path's cost)
    int32_t shift;              // screening fixed point: 2^-shift
    float scale;                // 2^-shift: screening sum -> approximate score
    unsigned int *next_col;
    eps_survivors *out;
    unsigned int *status;       // bit 1: a hash table filled up (cannot happen within the piece limits; backstop); bit 2: a column's
                                //        skipped head weighs as much as the bar (the head table was built for a higher bar: nothing valid);
                                //        bit 3: a sketch piece's set of reported ids filled up (the launch is void); bit 4: sketch pieces ran
    const uint4 *colrec;        // [n_columns][2] or NULL: what a column's set-up reads of five tables, in hand-out order (one 32-byte load
                                //        at the ticket's index instead of a chain id -> row start / head / row sum / plan pointer):
                                //        {v, rowptr[v], degree, head rows | head weight, row sum, first plan record, pieces}
    const uint32_t *rowrec;     // [n_nodes][32] or NULL: per node ONE 128-byte line with everything the walk wants of a row -- words
                                //        0..15 its 32 cuts, word 16 its first entry (rowptr), word 17 its screening weight (eps_scan_row_records)
    uint32_t wide_paths;        // r06, plans for sketch launches: a packed piece of a column of <= wide_rows rows may hold this many paths (it will
    int32_t wide_rows;          //      run as a sketch piece: no keys, no sum field -- only the unit bitmap's range bounds it); 0 = off
    uint32_t sketch;            // r06: PACKED pieces of single-round columns under a bar keep no keys (see SP_EM): 0 = off
    uint32_t batch_from;        // tickets below stand for one column, tickets from here on for SP_BATCH consecutive ones (>= n_columns: none)
    const uint4 *pack;          // [nnz][2] or NULL (r06; with plan + row records): per stored entry (v, j), in CSR order, everything a
                                //        single-round column's set-up gathers for it: {w, rowptr[w], fx32[w], revpos | cut of v's FIRST piece in
                                //        row w << 16} {cuts of v's pieces 1..8 in row w, 16 bits each} -- one contiguous stream per column
                                //        instead of neighbour ids -> one 128-byte row-record line per neighbour (eps_scan_column_pack)
    const uint2 *heads;         // [n_nodes] or NULL: column v does NOT walk its first heads[v].x rows (its heaviest hub neighbours under
                                //        hubs-first labels); heads[v].y = the sum of their screening weights.  See eps_scan_heads.
};

// Hash of an id: Fibonacci hashing.  The table index is taken from the TOP of the 32-bit product, the probe step from the
// middle, the pass of a partitioned window from the bottom.  (A full-rate 24 x 24-bit multiply was measured instead of the
// quarter-rate 32-bit one: its weaker mixing lengthens the probe sequences -- 38.0 vs 30.7 ms per launch.)
__device__ __forceinline__ uint32_t sp_mix(uint32_t x) { return x * 0x9E3779B1u; }
__device__ __forceinline__ uint32_t sp_mix2(uint32_t x) { return x * 0x85EBCA6Bu; }      // (the sketch pieces' second table)
// (2026-10-20: both slot indices of a sketch piece from ONE full-rate 24 x 24-bit multiply -- top bits and the bits below them -- were
//  measured against these two quarter-rate products: the main launch 6394 vs 6377 us, NOTES "Scan sweeps")

// The light zone of a main launch (scan_light.hip): columns [c0, c1) of p.colrec, one wave per column, tables of 2^bits_max words.  Appends to p.out and ORs into p.status like the piece kernel; draws its tickets on a counter of its own.
int sl_launch(const sp_params &p, uint32_t c0, uint32_t c1, int bits_max, hipStream_t stream);

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
