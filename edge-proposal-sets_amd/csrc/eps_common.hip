// Host-side plumbing of libeps_hip.so: thread-local error text, device query.
#include "eps_common.h"

#include <stdarg.h>
#include <string.h>

#include <atomic>

static thread_local char g_err[512] = "";

void eps_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *eps_last_error(void) { return g_err; }

extern "C" int eps_version(void) { return EPS_ABI_VERSION; }

int eps_num_cus()
{
    static thread_local int cached_dev = -1;
    static thread_local int cached_cus = 256;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != cached_dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cached_cus = n;
        cached_dev = dev;
    }
    return cached_cus;
}

extern "C" int eps_device_info(int *n_cu, char *name, int name_len)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        eps_set_error("eps_device_info: no HIP device");
        return EPS_ENODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        eps_set_error("eps_device_info: hipGetDeviceProperties failed");
        return EPS_ENODEV;
    }
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (name && name_len > 0) {
        snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    return EPS_OK;
}

// Work counters for the kernels that hand out work dynamically (one device word per launch): a small pool of device
// words inside the code object -- nothing is allocated at run time.  Each launch takes the next slot and zeroes it on
// its own stream before the kernel; 64 slots bound the number of such launches that may be in flight at once.
#define EPS_COUNTER_SLOTS 64
__device__ unsigned int g_work_counter[EPS_COUNTER_SLOTS];
static std::atomic<unsigned int> g_counter_turn{0};

int eps_take_counter(unsigned int **counter, hipStream_t stream, const char *who)
{
    if (hipGetSymbolAddress((void **)counter, HIP_SYMBOL(g_work_counter)) != hipSuccess) {
        eps_set_error("%s: cannot resolve the work counter", who);
        return EPS_ELAUNCH;
    }
    *counter += g_counter_turn.fetch_add(1) % EPS_COUNTER_SLOTS;
    if (hipMemsetAsync(*counter, 0, sizeof(unsigned int), stream) != hipSuccess) {
        eps_set_error("%s: cannot reset the work counter", who);
        return EPS_ELAUNCH;
    }
    return EPS_OK;
}

// Eight counters in one go (a hand-out sharded by XCD: eps_rescore_runs), zeroed on the caller's stream.
__device__ unsigned int g_work_counter8[EPS_COUNTER_SLOTS][8];
static std::atomic<unsigned int> g_counter8_turn{0};

int eps_take_counters8(unsigned int **counters, hipStream_t stream, const char *who)
{
    if (hipGetSymbolAddress((void **)counters, HIP_SYMBOL(g_work_counter8)) != hipSuccess) {
        eps_set_error("%s: cannot resolve the work counters", who);
        return EPS_ELAUNCH;
    }
    *counters += 8 * (g_counter8_turn.fetch_add(1) % EPS_COUNTER_SLOTS);
    if (hipMemsetAsync(*counters, 0, 8 * sizeof(unsigned int), stream) != hipSuccess) {
        eps_set_error("%s: cannot reset the work counters", who);
        return EPS_ELAUNCH;
    }
    return EPS_OK;
}

// ---- loading the library's code objects ahead of their first use ---------------------------------------------------------------
// The HIP runtime loads a translation unit's code object at the first launch of one of its kernels; a fresh process pays 10-30 ms
// for each of the larger ones (the rocPRIM sorts) inside whatever step happens to come first -- and filter.py is one fresh
// process per graph (submit_job.py:20-21).  eps_warm_up launches one empty kernel per unit on a stream of its own and waits for
// them: the host calls it from a background thread while the process is still reading its dataset.
// The units, once: every source of the library but this one (csrc/Makefile: SRCS) defines eps_warm_<unit>; the declarations
// and the calls below both come from this list (tests/test_abi.py holds it to SRCS).
#define EPS_UNITS(X) \
    X(graph_prep) X(csr_merge) X(scan_pieces) X(scan_light) X(scan_tables) X(scan_heads) X(rescore) \
    X(pair_intersect) X(pair_grouped) X(expand_score) X(filter_scan) X(spmm_csr) \
    X(gemm_f32) X(dense_cn) X(mlp_decode) X(mlp_decode_bf16) X(mlp_decode_train) X(topk_keys) X(topk_select) X(segment_topk) \
    X(tail_sort) X(rows_by_score) X(katz_pairs) X(katz_columns) X(local_index) X(cosine_cn) X(cosine_cn_bwd) X(pair_cn_list) X(local_community) X(sketch) \
    X(ppr_push) X(gat_attend)

#define EPS_DECLARE_WARM(unit) extern "C" void eps_warm_##unit(void *stream);
EPS_UNITS(EPS_DECLARE_WARM)

extern "C" int eps_warm_up(void)
{
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        eps_set_error("eps_warm_up: cannot create a stream");
        return EPS_ELAUNCH;
    }
#define EPS_CALL_WARM(unit) eps_warm_##unit(s);
    EPS_UNITS(EPS_CALL_WARM)
    const hipError_t e = hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    if (e != hipSuccess) {
        eps_set_error("eps_warm_up: %s", hipGetErrorString(e));
        return EPS_ELAUNCH;
    }
    return EPS_OK;
}
