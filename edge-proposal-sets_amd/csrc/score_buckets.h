// Order-preserving score buckets of the filter step's tail (tail_sort.hip: eps_score_hist / eps_score_pick_compact / eps_score_deal_plan;
// rows_by_score.hip: the cut read off a sorted list).  A bucket is a minifloat of a score's distance to a base score, in steps of the
// ordered bit pattern: 2^-TS_MB of that distance per bucket.  One definition: a cut derived in two places must be the same bits.
#pragma once
#include "eps_common.h"

#define TS_MB 8                                   // mantissa bits of the bucket minifloat
#define TS_BINS ((32 - TS_MB + 1) << TS_MB)       // 6400

// bucket of a distance d >= 0 (in steps of the ordered bit pattern): d itself below 2^MB, else exponent | top MB mantissa bits
__device__ __forceinline__ uint32_t ts_bucket(uint32_t d)
{
    if (d < (1u << TS_MB)) return d;
    const int e = 31 - __clz((int)d);                       // >= MB
    return ((uint32_t)(e - TS_MB + 1) << TS_MB) | ((d >> (e - TS_MB)) & ((1u << TS_MB) - 1u));
}
// smallest distance that falls into bucket b
__device__ __forceinline__ uint32_t ts_bucket_floor(uint32_t b)
{
    if (b < (1u << TS_MB)) return b;
    const uint32_t e1 = b >> TS_MB, m = b & ((1u << TS_MB) - 1u);
    return ((1u << TS_MB) | m) << (e1 - 1u);
}
