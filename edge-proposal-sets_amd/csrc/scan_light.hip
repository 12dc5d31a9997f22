// The lean kernel of the main scan launch's LIGHT columns, gfx950.
//
// What it replaces: nothing new -- the same part of filter.py:96-142 as scan_pieces.hip, for the columns whose whole walk is ONE
// sketch piece of a few rows (eps_amd.scan.light_split: one packed plan record, at most 64 rows, paths + known edges <= 2048).  In the
// piece kernel such a column is a dozen rows run by 256 threads behind eight workgroup barriers and a chain of dependent loads,
// four columns in flight per CU.  Here ONE WAVE is one column from ticket to report: no s_barrier anywhere, eight or nine columns in
// flight per CU (LDS: one table of 2^bits_max words per wave; the runtime's occupancy figure sizes the grid), the headers and plan records of a ticket's eight columns loaded together and
// the next column's pack lines in flight under the current column's walk.
//
// The semantics are the piece kernel's for a FULL && PACK && SK single-round sketch piece, to the bit: the same dead-column and
// bad-head tests, the same segments [0, min(cut, revpos)) of the rows past the skipped head, the same two hashes, shifts and half
// tables, the same gate (maximum of the first half table against bar - head weight), the same second look (min of the two slots,
// known neighbours out by binary search, every id reported once through a set -- one set per WAVE here, since a wave is a column).
// A report takes a single slot of the list (one global add): survivors are a handful per thousand such pieces, and the list keeps
// no holes below its counter.  The kernel adds nothing to n_candidates (sketch pieces do not count).
#include "eps_common.h"
#include "scan_common.h"
#include <string.h>
#include <atomic>

#define SL_BATCH 8              // consecutive light columns per ticket
#define SL_UNITS 1024           // units (of 4 entries) of the unit -> row bitmap: 2048 / 4 units + one ragged unit per row fit
#define SL_G 4                  // units a lane looks up and loads together before it consumes the first
#define SL_G2 2                 // ... in the second look (rare: registers go to the walk)
#define SL_ROWS 64              // rows of a light column at most (lane j holds row j)

// (a wave's own LDS traffic is in order; this only keeps the compiler from moving a phase's reads above the writes before it)
__device__ __forceinline__ void sl_lds_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

struct sl_unit {
    v4i u4;
    uint32_t fx;
    int nvalid;
};

__global__ __launch_bounds__(64, 3) void scan_light_kernel(sp_params p, uint32_t col0, uint32_t col1, int bits_max)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];      // [1 << bits_max] the two half tables of the column at hand
    const uint32_t words = 1u << bits_max;
    uint4 *r_desc = (uint4 *)(lds + words);              // [SL_ROWS] per dense row: first entry, entries, weight, first unit
    uint32_t *ubits = lds + words + 4 * SL_ROWS;         // [SL_UNITS / 32] bit s: a row starts at unit s
    uint32_t *wrank = ubits + SL_UNITS / 32;             // [SL_UNITS / 32] rows that start before the word
    uint32_t *em = wrank + SL_UNITS / 32;                // [SP_EM] id + 1 of every candidate the column has reported

    const int lane = threadIdx.x;
    const uint32_t out_cap = p.out->capacity;
    int64_t *__restrict__ out_key = p.out->key;
    float *__restrict__ out_val = p.out->val;
    const __amdgpu_buffer_rsrc_t col_rs = eps_raw_rsrc(p.col, p.col_bytes);
    const uint32_t thr32 = sp_bar_units(p.out->threshold, p.shift, false);
    if (thr32 >= SP_FLAG) {                              // (backstop: the host sends a light zone only under a bar -- without one the piece
        if (lane == 0) atomicOr(p.status, 2u);           //  kernel runs such a column as a packed piece and counts its candidates)
        return;
    }
    const uint32_t em_mask = (p.sketch >> 1 ? p.sketch >> 1 : (uint32_t)SP_EM) - 1u;

    for (uint32_t i = 4u * (uint32_t)lane; i < words; i += 256u) *(uint4 *)(lds + i) = make_uint4(0u, 0u, 0u, 0u);
    if (lane < SL_UNITS / 32) ubits[lane] = 0u;
    for (int i = lane; i < SP_EM; i += 64) em[i] = 0u;
    sl_lds_done();

    bool sketch_seen = false;
    const uint32_t n_tk = (col1 - col0 + SL_BATCH - 1u) / SL_BATCH;
    auto columns_of = [&](uint32_t tk) -> uint32_t {
        if (tk >= n_tk) return 0u;
        const uint32_t left = col1 - (col0 + tk * SL_BATCH);
        return left < (uint32_t)SL_BATCH ? left : (uint32_t)SL_BATCH;
    };
    // a ticket's headers: lanes 2 c and 2 c + 1 hold the two words of its column c (no ticket: zeros, and nothing below loads)
    auto load_headers = [&](uint32_t tk) {
        uint4 h = make_uint4(0u, 0u, 0u, 0u);
        if ((uint32_t)lane < 2u * columns_of(tk)) h = p.colrec[2 * ((size_t)col0 + (size_t)tk * SL_BATCH) + (size_t)lane];
        return h;
    };
    // ... lane c loads the one plan record of column c
    auto load_plan = [&](const uint4 &h, uint32_t nc) {
        const uint32_t pb_l = (uint32_t)__shfl((int)h.z, (2 * lane + 1) & 63);
        const uint32_t np_l = (uint32_t)__shfl((int)h.w, (2 * lane + 1) & 63);
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if ((uint32_t)lane < nc && np_l == 1u) r = p.plan[pb_l];
        return r;
    };
    // ... lane j loads the pack line of row j of column c
    auto pack_line = [&](const uint4 &h, uint32_t c) {
        const uint32_t vb = (uint32_t)__builtin_amdgcn_readlane((int)h.y, 2 * (int)c);
        const uint32_t dv = (uint32_t)__builtin_amdgcn_readlane((int)h.z, 2 * (int)c);
        uint4 pa = make_uint4(0u, 0u, 0u, 0u);
        if ((uint32_t)lane < dv && dv <= (uint32_t)SL_ROWS) pa = p.pack[2 * ((size_t)vb + (size_t)lane)];
        return pa;
    };
    uint32_t tk = blockIdx.x;
    while (tk < n_tk) {
        uint32_t tk_next = 0u;
        if (lane == 0) tk_next = gridDim.x + atomicAdd(p.next_col, 1u);      // in flight while this ticket's columns run
        const uint32_t nc = columns_of(tk);
        const uint4 hdr = load_headers(tk);
        const uint4 prec = load_plan(hdr, nc);
        uint4 pa_next = pack_line(hdr, 0u);
        for (uint32_t c = 0; c < nc; ++c) {
            const uint4 pa = pa_next;
            if (c + 1u < nc) pa_next = pack_line(hdr, c + 1u);      // (the next column's pack lines: in flight under this column's walk)
            const int c2 = 2 * (int)c;
            const int32_t v = __builtin_amdgcn_readlane((int)hdr.x, c2);
            const uint32_t vb = (uint32_t)__builtin_amdgcn_readlane((int)hdr.y, c2);
            const int32_t dv = __builtin_amdgcn_readlane((int)hdr.z, c2);
            const uint32_t xv = (uint32_t)__builtin_amdgcn_readlane((int)hdr.w, c2);
            const uint32_t hy = (uint32_t)__builtin_amdgcn_readlane((int)hdr.x, c2 + 1);
            const uint32_t ss = (uint32_t)__builtin_amdgcn_readlane((int)hdr.y, c2 + 1);
            const uint32_t np = (uint32_t)__builtin_amdgcn_readlane((int)hdr.w, c2 + 1);
            // a head as heavy as the bar: the head table was built for a higher one (status bit 2, the column is left out); a DEAD
            // column: its row sum lies below the bar
            bool out_of_it = hy >= thr32;
            const uint32_t thr_v = thr32 - hy;
            if (out_of_it && lane == 0) atomicOr(p.status, 4u);
            if (ss < thr32) out_of_it = true;
            if (dv <= 0 || v <= 0 || out_of_it || np == 0u) continue;
            const uint32_t info = (uint32_t)__builtin_amdgcn_readlane((int)prec.x, (int)c);
            const uint32_t nanb = (uint32_t)__builtin_amdgcn_readlane((int)prec.z, (int)c);
            const int na = (int)(nanb & 0xFFFFu), nb = (int)(nanb >> 16);
            const uint32_t pkeys = (info & 0x3FFFFFFFu) + (uint32_t)(nb - na);
            const int want = pkeys > 1u ? 33 - __clz((int)(pkeys - 1u)) : 1;      // smallest b with 2^b >= 2 * pkeys
            const int bits = want < 10 ? 10 : want;
            // (backstop: the host's split sends only single packed pieces of <= SL_ROWS rows whose table fits here)
            if (np != 1u || (info >> 30) != 1u || dv > SL_ROWS || bits > bits_max) {
                if (lane == 0) atomicOr(p.status, 2u);
                continue;
            }
            if (!sketch_seen && lane == 0) atomicOr(p.status, 16u);      // (informational: sketch pieces ran in this launch)
            sketch_seen = true;
            const int32_t *__restrict__ vcol = p.col + vb;

            // ---- describe: lane j = row j; its segment is [0, min(cut, revpos)) unless the head skips it
            uint32_t len = 0u;
            if (lane < dv) {
                const uint32_t rev = pa.w & 0xFFFFu, cut = pa.w >> 16;
                len = (uint32_t)lane < xv ? 0u : (cut < rev ? cut : rev);
            }
            const int units = (int)((len + 3u) >> 2);
            const int flag = units > 0 ? 1 : 0;
            const int incl_c = eps_wave_incl_scan_dpp(units | (flag << 24));
            const int incl = incl_c & 0xFFFFFF, incl_f = (int)((uint32_t)incl_c >> 24);
            const uint32_t a_u = (uint32_t)(incl - units);
            if (flag) {
                r_desc[incl_f - 1] = make_uint4(pa.y, len, pa.z, a_u);
                if (a_u < (uint32_t)SL_UNITS) atomicOr(&ubits[a_u >> 5], 1u << (a_u & 31u));
            }
            int total = __builtin_amdgcn_readlane(incl, 63);
            if (total > SL_UNITS) {                      // (backstop: <= 2048 paths in <= 64 rows are at most 576 units)
                if (lane == 0) atomicOr(p.status, 2u);
                total = SL_UNITS;
            }
            sl_lds_done();
            {
                const int cw = lane < SL_UNITS / 32 ? __popc(ubits[lane]) : 0;
                const int ex = eps_wave_incl_scan_dpp(cw) - cw;
                if (lane < SL_UNITS / 32) wrank[lane] = (uint32_t)ex;
            }
            sl_lds_done();

            // ---- walk: lane = one 4-entry unit, SL_G units per lane looked up and loaded together
            auto fetch_group = [&](int it0, auto &f) {
                constexpr int G = (int)(sizeof(f) / sizeof(f[0]));
                int lo[G];
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const uint32_t s = (uint32_t)((it0 + q) * 64 + lane);
                    const uint32_t wd = s < (uint32_t)SL_UNITS ? s >> 5 : 0u;
                    const uint32_t wbits = ubits[wd];
                    const int rk = (int)wrank[wd];
                    lo[q] = rk + __popc(wbits & ((2u << (s & 31u)) - 1u)) - 1;
                    lo[q] = lo[q] < 0 ? 0 : (lo[q] > SL_ROWS - 1 ? SL_ROWS - 1 : lo[q]);
                }
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const int s = (it0 + q) * 64 + lane;
                    const uint4 rd = r_desc[lo[q]];
                    f[q].fx = rd.z;
                    const bool in = s < total;
                    const int off = (s - (int)rd.w) * 4;
                    int left = (int)rd.y - off;
                    left = in ? left : 0;
                    f[q].nvalid = left < 0 ? 0 : (left > 4 ? 4 : left);
                    // (a unit past the end reads at an out-of-range offset of the buffer: zeros, no traffic)
                    const uint32_t at = in ? rd.x + (uint32_t)off : (p.col_bytes >> 2);
                    f[q].u4 = __builtin_amdgcn_raw_buffer_load_b128(col_rs, (int)(at * 4u), 0, 0);
                }
            };
            const int n_iter = (total + 63) >> 6;
            const uint32_t half = 1u << (bits - 1);
            for (int it0 = 0; it0 < n_iter; it0 += SL_G) {
                sl_unit f[SL_G];
                fetch_group(it0, f);
#pragma unroll
                for (int q = 0; q < SL_G; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < f[q].nvalid) {
                            const uint32_t id = (uint32_t)f[q].u4[e];
                            atomicAdd(&lds[sp_mix(id) >> (33 - bits)], f[q].fx);
                            atomicAdd(&lds[half + (sp_mix2(id) >> (33 - bits))], f[q].fx);
                        }
            }
            sl_lds_done();

            // ---- the gate: an id's estimate is at most its slot in the FIRST half table
            uint32_t mx = 0u;
            for (uint32_t i = 4u * (uint32_t)lane; i < half; i += 256u) {
                const uint4 a4 = *(const uint4 *)(lds + i);
                const uint32_t m01 = a4.x > a4.y ? a4.x : a4.y, m23 = a4.z > a4.w ? a4.z : a4.w;
                const uint32_t m = m01 > m23 ? m01 : m23;
                mx = m > mx ? m : mx;
            }
            const bool hot = __ballot(mx >= thr_v) != 0ull;
            if (hot) {
                // ---- the second look: min of the two slots per path; known neighbours out, every id once, a single slot per report
                auto report = [&](uint32_t u, uint32_t est) {
                    int a = na, b = nb;                   // a neighbour of v is no candidate (rows ascend: vcol[na, nb))
                    while (a < b) {
                        const int mid = (a + b) >> 1;
                        if (vcol[mid] < (int32_t)u) a = mid + 1; else b = mid;
                    }
                    if (a < nb && vcol[a] == (int32_t)u) return;
                    uint32_t h = (sp_mix(u) >> 9) & em_mask;
                    for (uint32_t tries = 0; tries <= em_mask; ++tries) {
                        const uint32_t old = atomicCAS(&em[h], 0u, u + 1u);
                        if (old == 0u) {                  // the first path of u that gets here reports it
                            const unsigned long long q = atomicAdd(&p.out->count, 1ull);
                            if (q < (unsigned long long)out_cap) {
                                out_key[q] = ((int64_t)v << 32) | (int64_t)u;
                                out_val[q] = __builtin_bit_cast(float, est);      // (the walked sum as it is: eps_scan_refine completes it)
                            }
                            return;
                        }
                        if (old == u + 1u) return;
                        h = (h + 1u) & em_mask;
                    }
                    atomicOr(p.status, 8u);               // the set is full: the launch is void (the host repeats it without sketch pieces)
                };
                for (int it0 = 0; it0 < n_iter; it0 += SL_G2) {
                    sl_unit f[SL_G2];
                    fetch_group(it0, f);
                    uint32_t est[4 * SL_G2];
#pragma unroll
                    for (int i = 0; i < 4 * SL_G2; ++i) {
                        const uint32_t id = (uint32_t)f[i >> 2].u4[i & 3];
                        const uint32_t ea = lds[sp_mix(id) >> (33 - bits)], eb = lds[half + (sp_mix2(id) >> (33 - bits))];
                        est[i] = ea < eb ? ea : eb;
                    }
#pragma unroll
                    for (int i = 0; i < 4 * SL_G2; ++i)
                        if ((i & 3) < f[i >> 2].nvalid && est[i] >= thr_v) report((uint32_t)f[i >> 2].u4[i & 3], est[i]);
                }
                sl_lds_done();
                for (int i = lane; i < SP_EM; i += 64) em[i] = 0u;
            }
            // ---- leave the table, the start bits (and, above, the set) clean for the next column
            for (uint32_t i = 4u * (uint32_t)lane; i < (1u << bits); i += 256u) *(uint4 *)(lds + i) = make_uint4(0u, 0u, 0u, 0u);
            if (lane < SL_UNITS / 32) ubits[lane] = 0u;
            sl_lds_done();
        }
        tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)tk_next);
    }
}

int sl_launch(const sp_params &p_in, uint32_t c0, uint32_t c1, int bits_max, hipStream_t stream)
{
    if (c1 <= c0) return EPS_OK;
    EPS_REQUIRE(bits_max >= 10 && bits_max <= 13, "eps_scan_screen: bad table size of the light zone");
    EPS_REQUIRE(p_in.colrec && p_in.plan && p_in.pack && p_in.sketch && p_in.out && p_in.status,
                "eps_scan_screen: the light zone needs column records, plan, pack and a sketch launch");
    sp_params p = p_in;
    unsigned int *counter = nullptr;
    const int rc = eps_take_counter(&counter, stream, "eps_scan_screen");
    if (rc) return rc;
    p.next_col = counter;
    const size_t lds = ((size_t)(1u << bits_max) + 4 * SL_ROWS + 2 * (SL_UNITS / 32) + SP_EM) * 4;
    // waves a CU holds at this LDS size, as the runtime counts them (its allocation granule decides between eight and nine at 4096
    // words): a block beyond that would wait for a wave to retire and then run its first ticket as a tail
    static std::atomic<int> per_cu_at[14];               // (asked once per table size)
    int per_cu = per_cu_at[bits_max].load();
    if (per_cu < 1) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)scan_light_kernel, 64, lds) != hipSuccess || per_cu < 1) {
            eps_set_error("eps_scan_screen: no occupancy figure for the light kernel at %zu bytes of LDS", lds);
            return EPS_ELAUNCH;
        }
        per_cu_at[bits_max].store(per_cu);
    }
    const int64_t tickets = ((int64_t)(c1 - c0) + SL_BATCH - 1) / SL_BATCH;
    int64_t blocks = (int64_t)eps_num_cus() * per_cu;
    if (blocks > tickets) blocks = tickets;
    hipLaunchKernelGGL(scan_light_kernel, dim3((unsigned)blocks), dim3(64), lds, stream, p, c0, c1, bits_max);
    EPS_CHECK_LAUNCH("eps_scan_screen");
    return EPS_OK;
}

// (one empty kernel per translation unit: launching it makes the HIP runtime load this unit's code object -- eps_warm_up)
__global__ void scan_light_warm_kernel() {}
extern "C" void eps_warm_scan_light(void *stream) { hipLaunchKernelGGL(scan_light_warm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream); }
