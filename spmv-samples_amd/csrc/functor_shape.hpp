// functor_shape.hpp — the launch shape of mi355_spmv_functor_spmv (functor_rtc.hip) as one pure host function: which of
// the rows kernels of functor_kernel.inc runs, on how many workgroups, what a long row is, and whether and how wide the
// long-row kernel launches.  No HIP in here: the host simulation of the kernels (tests/cpp/functor_sim.cpp) and the case
// table's checks (tests/functor_cases.py) read this rule instead of restating it.
#pragma once

#include <cstdint>

namespace mi355 {

// (functor_rtc.hip asserts that these are common.hpp's kBlock, kWave and kCus; the kernels' own are functor_kernel.inc's)
constexpr int kFunctorBlock = 256;
constexpr int kFunctorWave = 64;
constexpr int kFunctorCus = 256;                     // compute units per MI355X
constexpr int kFunctorLaneChoices = 6;               // T = 2, 4, 8, 16, 32, 64

struct FunctorShape {
    int choice;              // which rows kernel: mi355_functor_rows_<T>, T = 2 << choice
    int T;                   // lanes per row
    long long long_len;      // a row LONGER than this is left to mi355_functor_long_rows
    unsigned rows_grid;      // workgroups of the rows kernel
    bool long_launch;        // whether the long-row kernel launches at all
    unsigned long_grid;      // its workgroups (0 when it does not launch)
};

inline FunctorShape functor_shape(int32_t n_rows, int64_t nnz) {
    FunctorShape s;
    // lanes per row from the mean row length (the CSR-vector rule of the reference, cusp.cuh:203-221, on a 64-wide wave)
    // (a lane takes four nonzeros per step: T lanes cover a row of 4 T in one)
    const int64_t mean = nnz / n_rows;
    s.choice = 0;
    while (s.choice < kFunctorLaneChoices - 1 && (int64_t(8) << s.choice) < mean) ++s.choice;
    s.T = 2 << s.choice;
    s.long_len = 128ll * s.T;                        // (32 steps of the row's T lanes)
    if (s.long_len < 2048) s.long_len = 2048;
    const int rows_per_wg = kFunctorBlock / s.T;
    const int64_t want = (int64_t(n_rows) + rows_per_wg - 1) / rows_per_wg;
    s.rows_grid = unsigned(want < int64_t(kFunctorCus) * 32 ? want : int64_t(kFunctorCus) * 32);
    // the long rows: a row of that length only exists when nnz allows it
    s.long_launch = nnz > s.long_len;
    s.long_grid = 0;
    if (s.long_launch) {
        const int64_t waves = (int64_t(n_rows) + kFunctorWave - 1) / kFunctorWave;
        const int64_t wgs = (waves + kFunctorBlock / kFunctorWave - 1) / (kFunctorBlock / kFunctorWave);
        s.long_grid = unsigned(wgs < int64_t(kFunctorCus) * 8 ? wgs : int64_t(kFunctorCus) * 8);
    }
    return s;
}

}  // namespace mi355
