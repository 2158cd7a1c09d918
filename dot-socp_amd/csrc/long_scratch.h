// What the two-level transforms share (dct_long.hip for powers of two, cdft_long.hip for Bluestein's convolution): the
// complex scratch array in global memory between their passes and the LDS budget their tiles are cut to (each file
// names the bound of its own scratch array).
#pragma once
#include "fft_lds.h"
#include "solver.h"

#include <map>
#include <mutex>
#include <vector>

namespace dotsocp {

#define LONG_THREADS 256
#define LONG_BATCH 4                       // global loads in flight per lane before the first dependent LDS write
#define LONG_LDS_BUDGET (72 * 1024)        // two workgroups per CU
#define LONG_MAX_ROWS 32                   // staged rows per workgroup: divides LONG_THREADS

// The scratch arrays of one plan: one per stream (two launches of one plan may be in flight), from guarded_malloc, grown
// by replacement, freed with the plan.
struct LongScratch {
    std::mutex mu;
    struct Buf { double2 *p; size_t bytes; };
    std::map<hipStream_t, Buf> bufs;
    std::vector<double2 *> retired;        // outgrown arrays: work queued on them may still run, freed with the plan

    // the array of stream `st`, at least `bytes` long
    int get(hipStream_t st, size_t bytes, double2 **out) {
        std::lock_guard<std::mutex> lk(mu);
        Buf &b = bufs[st];
        if (b.bytes < bytes) {
            if (b.p) retired.push_back(b.p);
            b.p = nullptr;
            b.bytes = 0;
            DS_CHECK(guarded_malloc((void **)&b.p, bytes, true));       // complex doubles
            b.bytes = bytes;
        }
        *out = b.p;
        return 0;
    }
    void release() {
        for (auto &kv : bufs) dfree(kv.second.p);
        for (double2 *q : retired) dfree(q);
        bufs.clear();
        retired.clear();
    }
};

// log2 of the complex rows of length m a workgroup stages: what the LDS budget holds, at most LONG_MAX_ROWS
inline int long_log2_rows(int m) {
    i64 rows = (i64)(LONG_LDS_BUDGET / ((size_t)row_stride(m) * sizeof(double2)));
    if (rows > LONG_MAX_ROWS) rows = LONG_MAX_ROWS;
    if (rows < 2) rows = 2;
    return floor_log2(rows);
}

// exp(-2 pi i num / den), the index reduced exactly in integers
inline double2 unit_root(i64 num, i64 den) {
    const long double PI = 3.141592653589793238462643383279502884L;
    const long double a = -2.0L * PI * (long double)(num % den) / (long double)den;
    return make_double2((double)cosl(a), (double)sinl(a));
}

}  // namespace dotsocp
